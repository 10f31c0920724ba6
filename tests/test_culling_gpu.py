"""GPU parity: olf_keyframe_culling_tables_dev, olf_keyframe_culling, olf_tracked_map_points* and olf_map_point_culling* -- LocalMapping::KeyFrameCulling
(src/LocalMapping.cc:632-696) for a list of key frames against one snapshot of the map, KeyFrame::TrackedMapPoints / TrackedMapLines
(src/KeyFrame.cc:328-353, 407-432) and LocalMapping::MapPointCulling (:170-205).  Every comparison is exact equality of every output with the line-by-line
restatement (tests/culling_reference.py): the tables with its evaluation of every listed key frame as the map stands, the host form with its sequential
simulation.  The scenes (tests/culling_scenes.py) are the smallest at which each rule can go wrong.  The context is 320 x 240, the smallest image the batch
tests use."""
import functools
import subprocess
import numpy as np
import pytest
import culling_reference as R
import culling_scenes as S
import orb_line_slam_amd as ola
from orb_line_slam_amd import CullView, MapGraph, _lib, culling, localmap
from orb_line_slam_amd._lib import OLF_ERR_CAPACITY, OlfError

pytestmark = pytest.mark.gpu

STATUS_TEXT = {
    512: "a batched point entry left out a list index or a per-frame map-point index outside the map",
    1024: "a batched line entry left out a list index or a per-frame map-line index outside the map",
    4096: "a map-graph entry left out a key-frame index outside the graph",
    16384: "connected or ordered key-frame list of olf_update_connections_batch_dev, or a row of olf_best_covisibles_batch_dev",
}
SENTINEL, SENTINEL8, SLACK = -7, 200, 8
SEQUENCE_KEYS = ("decision", "n_mps", "n_redundant", "went_bad", "mp_nobs", "mp_bad")


@pytest.fixture(scope="module")
def ctx():
    import torch  # noqa: F401  (the device tensors below)
    p = _lib.default_params()
    p.orb.nfeatures = 300
    c = _lib.Context(p, 320, 240, 2)
    yield c
    c.close()


def up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def build(scene):
    graph = MapGraph(**scene.graph())
    return graph, CullView(graph, **scene.view())


def _status(ctx, bit):
    with pytest.raises(OlfError) as e:
        ctx.poll_status()
    assert e.value.code == OLF_ERR_CAPACITY and "flags=%d (%d: %s)" % (bit, bit, STATUS_TEXT[bit]) in str(e.value), str(e.value)
    ctx.poll_status()                                                # (read and cleared)


def run_tables(ctx, graph, view, kf_list, n_list, mono, capacity):
    """the device tables; returns a dict of numpy arrays.  Every output is SLACK longer than told and filled with a sentinel: nothing may be written past a
    list, a row or the capacity."""
    import torch
    i32 = lambda n: torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    u8 = lambda n: torch.full((n,), SENTINEL8, dtype=torch.uint8, device="cuda")
    out = dict(n_mps=i32(n_list + SLACK), n_redundant=i32(n_list + SLACK), redundant=u8(n_list + SLACK), row_offsets=i32(n_list + 1 + SLACK), slot_count=i32(capacity + SLACK),
               slot_flags=u8(capacity + SLACK))
    res = culling.keyframe_culling_tables_batch(graph, view, None if kf_list is None else up(np.asarray(kf_list, np.int32)), n_list=n_list, monocular=mono,
                                                slot_capacity=capacity, out=out, context=ctx)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def assert_tables(got, exp, n_list, capacity):
    for k, s in (("n_mps", SENTINEL), ("n_redundant", SENTINEL), ("redundant", SENTINEL8)):
        assert got[k][:n_list].tolist() == exp[k], k
        assert np.all(got[k][n_list:] == s), k + ": written past the list"
    assert got["row_offsets"][:n_list + 1].tolist() == exp["row_offsets"] and np.all(got["row_offsets"][n_list + 1:] == SENTINEL)
    m = min(exp["row_offsets"][-1], capacity)
    for k, s in (("slot_count", SENTINEL), ("slot_flags", SENTINEL8)):
        assert got[k][:m].tolist() == exp[k][:m], k
        assert np.all(got[k][m:] == s), k + ": written past the rows or the capacity"


def check_tables(ctx, scene, kf_list=None, mono=False, built=None):
    graph, view = build(scene) if built is None else built
    lst = list(range(scene.n_kf)) if kf_list is None else list(kf_list)
    exp = R.tables(scene.world(), lst, mono)
    cap = exp["row_offsets"][-1]
    assert cap == culling.listed_slots(graph, kf_list)
    got = run_tables(ctx, graph, view, kf_list, len(lst), mono, cap)
    assert_tables(got, exp, len(lst), cap)
    ctx.poll_status()
    return exp, (graph, view)


def check_host_form(ctx, scene, lst, mono=False):
    """KeyFrameCulling (tables on the device, replay on the host) against the sequential simulation and the tables' part against the evaluation"""
    graph, view = build(scene)
    got = ola.KeyFrameCulling(graph, view, lst, monocular=mono, context=ctx)
    sim = R.keyframe_culling(scene.world(), lst, mono)
    for k in SEQUENCE_KEYS:
        assert [int(v) for v in got[k]] == sim[k], k
    tab = R.tables(scene.world(), lst, mono)
    for k in ("n_mps", "n_redundant", "redundant"):
        assert got["table_" + k].tolist() == tab[k], k
    return sim, tab


@functools.lru_cache(maxsize=None)
def random_scene(n_kf, n_mp):
    return S.random_scene(1000 * n_kf + n_mp, n_kf, n_mp, max_obs=40 if n_mp == 300 else 12)


# ---- 1: random graphs ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("n_mp", [0, 40, 300])
@pytest.mark.parametrize("n_kf", [1, 2, 7, 65, 300])
def test_random_graphs(ctx, n_kf, n_mp, mono):
    scene = random_scene(n_kf, n_mp)
    exp, built = check_tables(ctx, scene, None, mono)
    lst = S.shuffled_list(n_kf + n_mp, n_kf)
    assert lst != sorted(lst) or n_kf <= 2
    assert len(set(lst)) < len(lst)
    check_tables(ctx, scene, lst, mono, built=built)
    if n_mp == 300 and n_kf >= 7:                                    # every kind of slot is there
        assert {0, 1, 3} <= set(exp["slot_flags"]) and max(exp["slot_count"]) > 3
    if n_mp == 300 and n_kf == 65 and not mono:
        assert exp["n_mps"] != R.tables(scene.world(), list(range(n_kf)), True)["n_mps"]      # (the depth test left slots out)


@pytest.mark.parametrize("n_kf, n_mp, max_obs, seed", [(40, 300, 6, 32), (60, 300, 5, 76)])
def test_dense_graphs_and_the_host_form(ctx, n_kf, n_mp, max_obs, seed):
    """graphs in which key frames are redundant and the list order matters in both directions (tests/test_culling_cpu.py chose the seeds)"""
    scene = S.random_scene(seed, n_kf, n_mp, max_obs=max_obs, dense=True)
    exp, _ = check_tables(ctx, scene)
    assert 0 < sum(exp["redundant"]) < n_kf
    lst = list(range(n_kf))
    sim, tab = check_host_form(ctx, scene, lst)
    assert any(t and d == 0 and scene.mode[k] == 0 for t, d, k in zip(tab["redundant"], sim["decision"], lst)) and any(not t and d for t, d in zip(tab["redundant"], sim["decision"]))
    check_host_form(ctx, scene, S.shuffled_list(seed, n_kf), mono=True)
    ctx.poll_status()


# ---- 2: lengths of a row: lane and chunk edges -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_slots", [0, 1, 63, 64, 65, 255, 256, 257, 1025])
def test_row_lengths(ctx, n_slots):
    scene = S.row_of(n_slots)
    exp, built = check_tables(ctx, scene, [0])
    assert exp["row_offsets"] == [0, n_slots]
    if n_slots >= 63:
        assert exp["n_redundant"][0] > 0 and exp["n_mps"][0] > exp["n_redundant"][0]
    check_tables(ctx, scene, [3, 0, 0, 6], built=built)              # the long row between short ones, twice


# ---- 3: lengths of an observation row: the in-flight group's edges --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_obs", [0, 1, 3, 4, 5, 40])
def test_observation_counts(ctx, n_obs):
    scene = S.observed_by(n_obs)
    exp, _ = check_tables(ctx, scene, [0])
    assert exp["slot_count"] == [sum(1 for k in range(1, n_obs + 1) if (k - 1) % 3 <= 1)] and exp["slot_flags"] == [3 if n_obs >= 4 else 1]


# ---- 4: the hand-worked scenes -----------------------------------------------------------------------------------------------------------------------------
def _hand_scenes():
    import test_culling_cpu as tc
    return tc.HAND_SCENES


@pytest.mark.parametrize("name", ["loses", "gains AB", "gains BA", "octave", "nobs 3", "nobs 4", "break", "mode 1", "mode 2", "twice", "stereo depths"])
def test_hand_scenes(ctx, name):
    make, want = _hand_scenes()[name]
    scene, lst = make()
    check_tables(ctx, scene, lst)
    sim, _ = check_host_form(ctx, scene, lst)
    assert {k: sim[k] for k in want} == want
    ctx.poll_status()


@pytest.mark.parametrize("n", S.BOUNDARY_N)
def test_the_09_boundary(ctx, n):
    for n_red in (n * 9 // 10, n * 9 // 10 + 1):
        scene, lst = S.boundary(n, n_red)
        exp, _ = check_tables(ctx, scene, lst)
        assert exp["redundant"] == [int(n_red > n * 9 // 10)]
        sim, _ = check_host_form(ctx, scene, lst)
        want = S.boundary_expected(n, n_red)
        assert {k: sim[k] for k in want} == want


def test_monocular(ctx):
    scene, lst = S.monocular_depths()
    for mono in (False, True):
        exp, _ = check_tables(ctx, scene, lst, mono)
        assert exp["n_mps"] == S.MONOCULAR_EXPECTED[int(mono)]["n_mps"]
        sim, _ = check_host_form(ctx, scene, lst, mono)
        want = S.MONOCULAR_EXPECTED[int(mono)]
        assert {k: sim[k] for k in want} == want


# ---- 5: nothing past a capacity; no list ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [0, 1, 100, 239])
def test_short_capacity_is_respected_and_reported(ctx, capacity):
    scene = random_scene(7, 300)
    graph, view = build(scene)
    lst = list(range(7))
    exp = R.tables(scene.world(), lst, False)
    assert exp["row_offsets"][-1] > 239
    got = run_tables(ctx, graph, view, None, 7, False, capacity)
    assert_tables(got, exp, 7, capacity)                             # the per-key-frame outputs and the offsets are complete
    _status(ctx, 16384)


def test_no_list_writes_nothing(ctx):
    scene, _ = S.loses_redundancy()
    graph, view = build(scene)
    got = run_tables(ctx, graph, view, None, 0, False, 4)
    for k, s in (("n_mps", SENTINEL), ("n_redundant", SENTINEL), ("row_offsets", SENTINEL), ("slot_count", SENTINEL), ("redundant", SENTINEL8), ("slot_flags", SENTINEL8)):
        assert np.all(got[k] == s), k
    ctx.poll_status()
    res = ola.KeyFrameCulling(graph, view, [], context=ctx)
    assert res["decision"].size == 0 and res["mp_nobs"].tolist() == scene.mp_nobs and res["went_bad"].size == 0


# ---- 6: malformed indices -------------------------------------------------------------------------------------------------------------------------------
def _malformed_base():
    scene = S.random_scene(77, 12, 200, max_obs=6, dense=True)
    exp = R.tables(scene.world(), list(range(12)), False)
    kf = next(k for k in range(12) if exp["n_redundant"][k] > 3)
    slot = next(i for i in range(len(scene.kf_mp[kf])) if exp["slot_flags"][exp["row_offsets"][kf] + i] == 3)
    return scene, kf, slot


def _check_malformed(ctx, scene, graph, view, lst, bit):
    """the device against the restatement on the malformed world, which leaves out what include/orbline.h says; exactly `bit` is raised"""
    w = scene.world()
    w["n_mp"] = graph.n_mp                                           # (a test may have shrunk the map under the slots)
    exp = R.tables(w, lst, False)
    assert R.status_bits(w, lst, False) == bit
    got = run_tables(ctx, graph, view, lst, len(lst), False, exp["row_offsets"][-1])
    assert_tables(got, exp, len(lst), exp["row_offsets"][-1])
    _status(ctx, bit)
    return exp


def test_malformed_slot_index(ctx):
    scene, kf, slot = _malformed_base()
    clean = R.tables(scene.world(), [kf], False)
    graph, view = build(scene)
    scene.kf_mp[kf][slot] = scene.n_mp + 5                           # past the map: MapGraph would refuse it, so it goes into the built arrays
    graph.kf_mp_index[graph.kf_mp_offsets[kf] + slot] = scene.n_mp + 5
    exp = _check_malformed(ctx, scene, graph, view, [kf], 512)
    assert exp["n_mps"][0] == clean["n_mps"][0] - 1 and exp["n_redundant"][0] == clean["n_redundant"][0] - 1 and exp["slot_flags"][slot] == 0


def test_malformed_observing_key_frame(ctx):
    scene, kf, slot = _malformed_base()
    clean = R.tables(scene.world(), [kf], False)
    p = scene.kf_mp[kf][slot]
    o = next(i for i, (k, _) in enumerate(scene.mp_obs[p]) if k != kf and scene.kf_oct[k][scene.mp_obs[p][i][1]] <= scene.kf_oct[kf][slot] + 1)
    graph, view = build(scene)
    for bad_kf in (scene.n_kf, -1, 1 << 30):
        scene.mp_obs[p][o][0] = bad_kf
        graph.mp_obs_kf[graph.mp_obs_offsets[p] + o] = bad_kf
        graph._dev = None
        exp = _check_malformed(ctx, scene, graph, view, [kf], 4096)
        assert exp["slot_count"][slot] == clean["slot_count"][slot] - 1


def test_malformed_observation_slot(ctx):
    scene, kf, slot = _malformed_base()
    clean = R.tables(scene.world(), [kf], False)
    p = scene.kf_mp[kf][slot]
    o = next(i for i, (k, _) in enumerate(scene.mp_obs[p]) if k != kf and scene.kf_oct[k][scene.mp_obs[p][i][1]] <= scene.kf_oct[kf][slot] + 1)
    observer = scene.mp_obs[p][o][0]
    graph, view = build(scene)
    for bad_slot in (len(scene.kf_mp[observer]), -1, 1 << 30):
        scene.mp_obs[p][o][1] = bad_slot
        view.mp_obs_slot[graph.mp_obs_offsets[p] + o] = bad_slot
        view._dev = None
        exp = _check_malformed(ctx, scene, graph, view, [kf], 4096)
        assert exp["slot_count"][slot] == clean["slot_count"][slot] - 1
    # the listed key frame's own observation is skipped before its slot is looked at: no bit
    scene, kf, slot = _malformed_base()
    p = scene.kf_mp[kf][slot]
    own = next(i for i, (k, _) in enumerate(scene.mp_obs[p]) if k == kf)
    scene.mp_obs[p][own][1] = 1 << 20
    assert R.status_bits(scene.world(), [kf], False) == 0
    check_tables(ctx, scene, [kf])


def test_malformed_listed_key_frame(ctx):
    scene, kf, _ = _malformed_base()
    graph, view = build(scene)
    lst = [kf, scene.n_kf, -1, 1 << 30, kf]
    exp = _check_malformed(ctx, scene, graph, view, lst, 4096)
    assert exp["n_mps"][1:4] == [0, 0, 0] and exp["row_offsets"][1] == exp["row_offsets"][4] and exp["n_mps"][0] == exp["n_mps"][4] > 0
    with pytest.raises(OlfError) as e:                               # the host form: OLF_ERR_CAPACITY with the bit's text
        ola.KeyFrameCulling(graph, view, lst, context=ctx)
    assert e.value.code == OLF_ERR_CAPACITY and STATUS_TEXT[4096] in str(e.value)


# ---- 7: TrackedMapPoints / TrackedMapLines ---------------------------------------------------------------------------------------------------------------
def _tracked_expected(scene, lst, min_p, min_l):
    pts = [R.tracked(scene.kf_mp[k], scene.mp_bad, scene.mp_nobs, min_p) if 0 <= k < scene.n_kf else 0 for k in lst]
    lines = [R.tracked(scene.kf_ml[k], scene.ml_bad, scene.ml_nobs, min_l) if 0 <= k < scene.n_kf and scene.kf_ml is not None else 0 for k in lst]
    return pts, lines


@pytest.mark.parametrize("min_p, min_l", [(0, 0), (-1, 3), (3, 1), (1, 0), (4, 4)])
@pytest.mark.parametrize("n_kf, n_mp", [(1, 0), (7, 40), (65, 300)])
def test_tracked_map_points(ctx, n_kf, n_mp, min_p, min_l):
    import torch
    scene = S.with_lines(S.random_scene(5 + n_kf, n_kf, n_mp), seed=n_kf)
    graph = MapGraph(**scene.graph())
    lst = [-1] + S.shuffled_list(3, n_kf) + [-1]
    want = _tracked_expected(scene, lst, min_p, min_l)
    out = dict(n_points=torch.full((len(lst) + SLACK,), SENTINEL, dtype=torch.int32, device="cuda"), n_lines=torch.full((len(lst) + SLACK,), SENTINEL, dtype=torch.int32, device="cuda"))
    res = culling.tracked_map_points_batch(graph, up(np.asarray(scene.mp_nobs, np.int32)) if n_mp else None, up(np.asarray(lst, np.int32)),
                                           ml_nobs=up(np.asarray(scene.ml_nobs, np.int32)), min_obs_points=min_p, min_obs_lines=min_l, out=out, context=ctx)
    torch.cuda.synchronize()
    for k, w in zip(("n_points", "n_lines"), want):
        got = res[k].cpu().numpy()
        assert got[:len(lst)].tolist() == w and np.all(got[len(lst):] == SENTINEL), k
    ctx.poll_status()                                                # -1 is "no reference key frame": no bit
    host = ola.TrackedMapPoints(graph, scene.mp_nobs, lst, ml_nobs=scene.ml_nobs, min_obs_points=min_p, min_obs_lines=min_l, context=ctx)
    assert host[0].tolist() == want[0] and host[1].tolist() == want[1]
    if n_mp == 300 and min_p == 4:                                   # (a point that is not bad has at least 3: the test bites from 4 on)
        assert want[0] != _tracked_expected(scene, lst, 0, 0)[0] and any(want[0]) and any(want[1]) and want[1] != _tracked_expected(scene, lst, 0, 0)[1]


def test_tracked_map_points_without_lines_and_out_of_range(ctx):
    import torch
    scene = S.random_scene(9, 7, 40)
    graph = MapGraph(**scene.graph())
    lst = [0, 7, -1, 3, -2]
    want = _tracked_expected(scene, lst, 2, 0)
    res = culling.tracked_map_points_batch(graph, up(np.asarray(scene.mp_nobs, np.int32)), up(np.asarray(lst, np.int32)), min_obs_points=2, context=ctx)
    torch.cuda.synchronize()
    assert res["n_points"].cpu().tolist() == want[0] and res["n_lines"].cpu().tolist() == [0] * 5 and want[0][1] == 0 and want[0][0] > 0
    _status(ctx, 4096)                                               # 7 and -2 are outside the graph; -1 alone raises nothing
    res = culling.tracked_map_points_batch(graph, None, None, n_list=7, context=ctx)      # no list: every key frame; no observation test
    torch.cuda.synchronize()
    assert res["n_points"].cpu().tolist() == _tracked_expected(scene, range(7), 0, 0)[0]
    ctx.poll_status()


def test_tracked_map_points_of_the_reference_key_frames(ctx):
    """ref_kf of update_local_map_batch, a device tensor, goes in as it is -- its -1 included (Tracking::NeedNewKeyFrame, src/Tracking.cc:1626-1627)"""
    import torch
    import connections_scenes as CS
    import test_localmap_gpu as tl
    scene = CS.random_graph(3, 65, 300, n_frames=17, max_obs=8)
    scene.frame_mp.append([-1, -1])                                  # a frame that holds nothing: no reference key frame
    graph = MapGraph(**scene.graph())
    fmp, cnt = tl.rows(ctx, scene.frame_mp, ctx.orb_capacity, 1, 0)
    out = localmap.update_local_map_batch(graph, len(scene.frame_mp), up(fmp), up(cnt), context=ctx)
    rng = np.random.default_rng(1)
    mp_nobs = rng.integers(0, 7, size=300).astype(np.int32)
    res = culling.tracked_map_points_batch(graph, up(mp_nobs), out["ref_kf"], min_obs_points=3, context=ctx)
    torch.cuda.synchronize()
    ref = out["ref_kf"].cpu().tolist()
    assert ref[-1] == -1 and max(ref) >= 0
    g = scene.graph()
    want = [R.tracked(g["kf_mp"][k], g["mp_bad"], mp_nobs, 3) if k >= 0 else 0 for k in ref]
    assert res["n_points"].cpu().tolist() == want and any(want)
    try:                                                             # (the local-map lists had no capacity: that call's own bit, read and cleared)
        ctx.poll_status()
    except OlfError as e:
        assert "flags=8192 " in str(e)


# ---- 8: MapPointCulling ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mono", [False, True])
@pytest.mark.parametrize("n", [0, 1, 64, 65, 1000])
def test_map_point_culling(ctx, n, mono):
    import torch
    a = S.recent_points(n, n)
    want = R.map_point_culling(a["bad"], a["found"], a["visible"], a["nobs"], a["first_kf_id"], a["current_kf_id"], mono)
    if n >= 64:
        assert want[:12] == S.RECENT_FIXED_ACTIONS[int(mono)] and set(want) == {0, 1, 2, 3, 4}
        assert a["visible"][3] == 0 and a["visible"][4] == 0 and a["found"][2] * 4 == a["visible"][2]
    out = torch.full((n + SLACK,), SENTINEL8, dtype=torch.uint8, device="cuda")
    res = culling.map_point_culling(up(a["bad"]), up(a["found"]), up(a["visible"]), up(a["nobs"]), up(a["first_kf_id"]), a["current_kf_id"], mono, out=out, context=ctx)
    torch.cuda.synchronize()
    got = res.cpu().numpy()
    assert got[:n].tolist() == want and np.all(got[n:] == SENTINEL8)
    host = ola.MapPointCulling(a["bad"], a["found"], a["visible"], a["nobs"], a["first_kf_id"], a["current_kf_id"], mono, context=ctx)
    assert host.tolist() == want
    ctx.poll_status()


def test_map_point_culling_takes_the_id_difference_in_int(ctx):
    got = ola.MapPointCulling([0, 0], [4, 4], [4, 4], [9, 9], [1, 1 << 32], (1 << 32) + 5, context=ctx)
    assert got.tolist() == R.map_point_culling([0, 0], [4, 4], [4, 4], [9, 9], [1, 1 << 32], (1 << 32) + 5, False) == [4, 4]


# ---- 9: the reference-side adaptor on the device ---------------------------------------------------------------------------------------------------------
def test_adaptor_keyframe_culling(tmp_path):
    from test_culling_cpu import build_adaptor
    exe = str(tmp_path / "adaptor_culling")
    build_adaptor(exe)
    out = subprocess.run([exe, "device"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_CULLING_OK" in out.stdout, out.stdout.decode()[-3000:]
