"""olf_initializer_pairs_dev and olf_initializer_apply_dev on the device against the host form olf_initializer, bit for bit on every output (one header,
no contraction; NaNs compared as one pattern), over the scenes of tests/initializer_scenes.py at the context's capacity of 512: every row of the scene
table under the three parameter sets, the pair list permuted, the scratch-slot placement of the correspondences against the LDS one, sentinels in
everything the call must leave, refused pairs, n_pairs == 0, the host-pointer form, olf_initializer_apply_dev against numpy (in place and out of place),
the adaptor's batched function, and the chain olf_search_for_initialization -> initialiser -> apply on one synthetic pair, the matcher's row read as it is.  At most 21 pairs per call:
the grid stride over more than 1024 pairs is not exercised here."""
import numpy as np
import pytest
import initializer_scenes as S
import orb_line_slam_amd as ola
from orb_line_slam_amd import _lib
from test_initializer_cpu import host_solve, sentinel_state

pytestmark = pytest.mark.gpu
F = np.float32
KEYS = tuple(k for k, _, _ in ola.initializer._STATE)


@pytest.fixture(scope="module")
def ctx():
    p = _lib.default_params()
    p.orb.nfeatures = 448
    c = _lib.Context(p, 320, 240, 2)
    assert c.orb_capacity == S.CAP
    yield c
    _lib.lib().olf_debug_initializer_lds_limit(0)
    c.close()


def up(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype.fields:
        a = a.view(np.uint8).reshape(a.shape + (-1,))
    return torch.from_numpy(a).cuda()


def _bits(v):
    v = np.ascontiguousarray(v)
    if v.dtype != np.float32:
        return v
    return np.where(np.isnan(v), np.uint32(0x7fc00000), v.view(np.uint32))


def same_state(a, b):
    for k in KEYS:
        x, y = _bits(a[k]), _bits(b[k])
        assert np.array_equal(x, y), (k, np.argwhere(x != y)[:6])


def device_solve(ctx, pset, names, order=None):
    """olf_initializer_pairs_dev over the scenes `names` in `order`; returns the state as host arrays in the scenes' order"""
    import torch
    kps, counts, pairs, matches = S.batch(names)
    prm = ola.initializer_params(**S.SETS[pset])
    order = list(range(len(names))) if order is None else list(order)
    st = sentinel_state(len(names), S.CAP)
    d = {k: up(st[k][order]) for k in KEYS}
    dr = np.stack([S.draws(n, prm.max_iterations) for n in names])
    ola.initializer_batch(2 * len(names), up(kps), up(counts), S.CAM, up(pairs[order]), up(matches[order]), up(dr[order]), d, prm, img_stride=1, context=ctx)
    torch.cuda.synchronize()
    ctx.poll_status()
    for k in KEYS:
        st[k][order] = d[k].cpu().numpy()
    return st


@pytest.fixture(scope="module")
def host():
    return {pset: host_solve(pset) for pset in ("fast", "tracker", "one")}


@pytest.mark.parametrize("pset", ["fast", "tracker", "one"])
def test_device_equals_the_host_form(ctx, host, pset):
    names, st, bits = host[pset]
    assert bits == 0
    dev = device_solve(ctx, pset, names)
    same_state(dev, st)
    if pset == "fast":
        assert list(st["n_correspondences"][:12]) == [0, 7, 8, 9, 63, 64, 65, 255, 256, 257, S.CAP, 300] and st["ok"].sum() >= 12
        # what the call must leave: rows past the reference frame's count, H21 / R21 / P3D of a pair without them
        for p, n in enumerate(names):
            N1 = min(int(S.scene(n).counts[0]), S.CAP)
            assert (dev["inliers_H"][p, N1:] == 77).all() and (dev["inliers_F"][p, N1:] == 77).all() and (dev["triangulated"][p, N1:] == 77).all()
            if dev["ok"][p] <= 0:
                assert (dev["R21"][p] == -7).all() and (dev["P3D"][p] == -7).all() and (dev["triangulated"][p] == 77).all()


def test_permuted_pairs(ctx, host):
    names, st, _ = host["fast"]
    same_state(device_solve(ctx, "fast", names, order=np.random.default_rng(3).permutation(len(names))), st)


def test_scratch_placement(ctx, host):
    names, st, _ = host["fast"]
    assert _lib.lib().olf_debug_initializer_lds_limit(1024) == 0     # 32 * 512 bytes do not fit: the correspondences live in context scratch
    try:
        same_state(device_solve(ctx, "fast", names), st)
    finally:
        _lib.lib().olf_debug_initializer_lds_limit(0)


def test_refused_pairs_nothing_and_the_staged_form(ctx, host):
    import torch
    names, st, _ = host["fast"]
    sub = ["general", "planar", "n7"]
    kps, counts, pairs, matches = S.batch(sub)
    prm = ola.initializer_params(**S.FAST)
    dr = np.stack([S.draws(n, prm.max_iterations) for n in sub])
    # refused pairs among good ones
    bad = np.array([[0, 1], [3, 3], [-1, 2], [4, 6]], np.int32)
    s4 = sentinel_state(4, S.CAP)
    d = {k: up(s4[k]) for k in KEYS}
    ola.initializer_batch(6, up(kps), up(counts), S.CAM, up(bad), up(np.stack([matches[0]] * 4)), up(np.stack([dr[0]] * 4)), d, prm, img_stride=1, context=ctx)
    torch.cuda.synchronize()
    with pytest.raises(ola.OlfError):
        ctx.poll_status()                                            # bit 2048
    got = {k: d[k].cpu().numpy() for k in KEYS}
    assert list(got["ok"][1:]) == [-1, -1, -1] and got["ok"][0] == st["ok"][names.index("general")]
    for k in KEYS:
        if k != "ok":
            assert (got[k][1:] == (77 if got[k].dtype == np.uint8 else -7)).all(), k
    # n_pairs == 0 writes nothing
    d = {k: up(s4[k]) for k in KEYS}
    ola.initializer_batch(6, up(kps), up(counts), S.CAM, up(bad[:0]), up(matches[:0]), up(dr[:0]), d, prm, img_stride=1, context=ctx)
    torch.cuda.synchronize()
    same_state({k: d[k].cpu().numpy() for k in KEYS}, s4)
    # the host-pointer form
    s3 = sentinel_state(3, S.CAP)
    ola.initializer_pairs(kps, counts, S.CAM, pairs, matches, dr, s3, prm, context=ctx)
    same_state(s3, {k: st[k][[names.index(n) for n in sub]] for k in KEYS})


def test_adaptor_on_the_device(tmp_path):
    """tests/adaptor_initializer.cpp with `device`: a vector of initialisers through InitializersInitialize on the thread's context, bit for bit the host form's"""
    import subprocess
    from test_initializer_cpu import build_adaptor
    exe = str(tmp_path / "adaptor_initializer")
    build_adaptor(exe)
    out = subprocess.run([exe, "device"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_INITIALIZER_OK" in out.stdout, out.stdout.decode()[-3000:]


def test_apply_and_the_chain_from_the_matcher(ctx, host):
    import torch
    names, st, _ = host["fast"]
    kps, counts, pairs, matches = S.batch(names)
    d = {k: up(st[k]) for k in KEYS}
    out, nm, Tcw = ola.initializer_apply(2 * len(names), up(counts), up(pairs), up(matches), d, out=torch.full(matches.shape, -9, dtype=torch.int32, device="cuda"),
                                         n_matches=torch.full((len(names),), -9, dtype=torch.int32, device="cuda"),
                                         Tcw=torch.full((len(names), 16), -9.0, device="cuda"), img_stride=1, context=ctx)
    inplace = up(matches)
    ola.initializer_apply(2 * len(names), up(counts), up(pairs), inplace, d, out=inplace, img_stride=1, context=ctx)
    torch.cuda.synchronize()
    out, nm, Tcw, inplace = out.cpu().numpy(), nm.cpu().numpy(), Tcw.cpu().numpy(), inplace.cpu().numpy()
    for p, n in enumerate(names):
        if st["ok"][p] <= 0:                                         # rows of pairs that did not initialise stay
            assert (out[p] == -9).all() and nm[p] == -9 and (Tcw[p] == -9).all() and np.array_equal(inplace[p], matches[p]), n
            continue
        N1, N2 = (min(int(c), S.CAP) for c in S.scene(n).counts)
        i = np.arange(S.CAP)
        on = (i < N1) & (matches[p] >= 0) & (matches[p] < N2) & (st["triangulated"][p] == 1)      # Tracking.cc:758-765
        want = np.where(on, matches[p], -1)
        assert np.array_equal(out[p], want) and np.array_equal(inplace[p], want) and nm[p] == on.sum(), n
        T = np.eye(4, dtype=F)
        T[:3, :3], T[:3, 3] = st["R21"][p].reshape(3, 3), st["t21"][p]
        assert np.array_equal(Tcw[p].reshape(4, 4), T), n
    # the chain on one synthetic pair: descriptors that match one to one, the matcher's row as it is (padded to the capacity with its own -1)
    s = S.scene("general")
    rng = np.random.default_rng(9)
    N1, N2 = int(s.counts[0]), int(s.counts[1])
    kp = s.kp.copy()
    kp["octave"] = 0
    desc1 = rng.integers(0, 256, (N1, 32), dtype=np.uint8)
    desc2 = rng.integers(0, 256, (N2, 32), dtype=np.uint8)
    m = s.matches[:N1]
    good = (m >= 0) & (m < N2)
    desc2[m[good]] = desc1[good]
    view = dict(fx=S.CAM[0], fy=S.CAM[1], cx=S.CAM[2], cy=S.CAM[3], bounds=(0.0, 640.0, 0.0, 480.0))
    F1, F2 = ola.FrameView(kp[0, :N1], desc1, **view), ola.FrameView(kp[1, :N2], desc2, **view)
    prev = np.ascontiguousarray(np.stack([kp["x"][0, :N1], kp["y"][0, :N1]], 1), F)
    n, row = ola.ORBmatcher(0.9, True).SearchForInitialization(F1, F2, prev, 100)
    assert n >= 150
    full = np.full((1, S.CAP), -1, np.int32)
    full[0, :N1] = row
    prm = ola.initializer_params(**S.FAST)
    dr = S.draws("general", prm.max_iterations)[None]
    hs = sentinel_state(1, S.CAP)
    assert ola.Initialize(kp, s.counts, S.CAM, (0, 1), full[0], dr[0], hs, prm) == 0 and hs["ok"][0] == 1
    d = {k: up(v) for k, v in sentinel_state(1, S.CAP).items()}
    pr = np.array([[0, 1]], np.int32)
    ola.initializer_batch(2, up(kp), up(s.counts), S.CAM, up(pr), up(full), up(dr), d, prm, img_stride=1, context=ctx)
    out, nm, Tcw = ola.initializer_apply(2, up(s.counts), up(pr), up(full), d, img_stride=1, context=ctx)
    torch.cuda.synchronize()
    ctx.poll_status()
    same_state({k: d[k].cpu().numpy() for k in KEYS}, hs)
    assert int(nm[0]) == int(hs["triangulated"][0][:N1][row >= 0].sum()) >= 100
    assert np.array_equal(out.cpu().numpy()[0, :N1], np.where(hs["triangulated"][0][:N1] == 1, row, -1))
