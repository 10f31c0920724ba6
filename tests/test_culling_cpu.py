"""LocalMapping::KeyFrameCulling, MapPointCulling and KeyFrame::TrackedMapPoints without a device: the restatement (tests/culling_reference.py) against
answers worked out by hand from src/LocalMapping.cc:632-696 and printed beside the scenes (tests/culling_scenes.py); olf_keyframe_culling_replay, fed the
restatement's tables, against the restatement's sequential simulation on the hand scenes and on random graphs in which the list order matters in both
directions; the argument checks of the seven C entries; the exports; and the reference-side adaptor (include/orbline_reference_api.hpp) compiled against
stand-in types and run on its replay path."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import culling_reference as R
import culling_scenes as S
from orb_line_slam_amd import CullView, MapGraph, _lib, culling
from orb_line_slam_amd._lib import OLF_ERR_INVALID, last_error, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQUENCE_KEYS = ("decision", "n_mps", "n_redundant", "went_bad")
HAND_SCENES = {
    "loses": (S.loses_redundancy, S.LOSES_EXPECTED), "gains AB": (lambda: S.gains_redundancy("AB"), S.GAINS_EXPECTED["AB"]),
    "gains BA": (lambda: S.gains_redundancy("BA"), S.GAINS_EXPECTED["BA"]), "octave": (S.octave_rule, S.OCTAVE_EXPECTED),
    "nobs 3": (lambda: S.nobs_boundary(0), S.NOBS_EXPECTED[0]), "nobs 4": (lambda: S.nobs_boundary(1), S.NOBS_EXPECTED[1]), "break": (S.break_irrelevance, S.BREAK_EXPECTED),
    "mode 1": (lambda: S.modes(1), S.MODES_EXPECTED[1]), "mode 2": (lambda: S.modes(2), S.MODES_EXPECTED[2]), "twice": (S.listed_twice, S.TWICE_EXPECTED),
    "stereo depths": (S.monocular_depths, S.MONOCULAR_EXPECTED[0]),
}


def subset(d, keys):
    return {k: [int(v) for v in d[k]] for k in keys}


# ---- the restatement against hand-worked answers -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(HAND_SCENES))
def test_simulation_of_the_hand_scenes(name):
    make, exp = HAND_SCENES[name]
    scene, lst = make()
    assert subset(R.keyframe_culling(scene.world(), lst, False), SEQUENCE_KEYS) == exp


def test_tables_of_the_two_order_scenes():
    """as the map stands, before anything is culled: what the replay starts from"""
    scene, lst = S.loses_redundancy()
    assert subset(R.tables(scene.world(), lst, False), S.LOSES_TABLES) == S.LOSES_TABLES
    for order in ("AB", "BA"):
        scene, lst = S.gains_redundancy(order)
        assert subset(R.tables(scene.world(), lst, False), S.GAINS_TABLES[order]) == S.GAINS_TABLES[order]
    # the order effects themselves: redundant by the tables and kept; not redundant by the tables and culled
    assert S.LOSES_TABLES["redundant"][1] == 1 and S.LOSES_EXPECTED["decision"][1] == 0
    assert S.GAINS_TABLES["AB"]["redundant"][1] == 0 and S.GAINS_EXPECTED["AB"]["decision"][1] == 1


@pytest.mark.parametrize("n", S.BOUNDARY_N)
def test_the_09_boundary(n):
    for n_red in (n * 9 // 10, n * 9 // 10 + 1):
        scene, lst = S.boundary(n, n_red)
        assert subset(R.keyframe_culling(scene.world(), lst, False), SEQUENCE_KEYS) == S.boundary_expected(n, n_red), (n, n_red)
    assert float(n * 9 // 10) == 0.9 * float(n)                      # the product is the integer itself: equality is "not greater"


def test_octave_rule_and_break_tables():
    for make, tab in ((S.octave_rule, S.OCTAVE_TABLES), (S.break_irrelevance, S.BREAK_TABLES)):
        scene, lst = make()
        assert subset(R.tables(scene.world(), lst, False), tab) == tab


def test_nobs_boundary_keeps_the_count():
    for extra in (0, 1):
        scene, lst = S.nobs_boundary(extra)
        t = R.tables(scene.world(), lst, False)
        assert t["slot_count"] == [3] and t["slot_flags"] == [1 + 2 * extra]


def test_monocular_counts_far_and_negative_depths():
    scene, lst = S.monocular_depths()
    for mono in (0, 1):
        assert subset(R.keyframe_culling(scene.world(), lst, bool(mono)), SEQUENCE_KEYS) == S.MONOCULAR_EXPECTED[mono]


def test_map_point_culling_restatement():
    a = S.recent_points(0, 12)
    for mono in (0, 1):
        got = R.map_point_culling(a["bad"], a["found"], a["visible"], a["nobs"], a["first_kf_id"], a["current_kf_id"], mono)
        assert got == S.RECENT_FIXED_ACTIONS[mono]
        assert set(got) == {0, 1, 2, 3, 4}
    # the id difference is taken in int: an id beyond 2^31 wraps as the casts at :195, :200 do
    assert R.map_point_culling([0], [4], [4], [9], [1], (1 << 32) + 5, 0) == [4] and R.map_point_culling([0], [4], [4], [9], [1], (1 << 31) + 5, 0) == [0]


def test_tracked_restatement():
    row, bad, nobs = [0, -1, 1, 2, 3, 0], [0, 0, 1, 0], [3, 2, 9, 1]
    assert R.tracked(row, bad, nobs, 0) == 4 and R.tracked(row, bad, nobs, -1) == 4      # points 0, 1, 3 and 0 again
    assert R.tracked(row, bad, nobs, 2) == 3 and R.tracked(row, bad, nobs, 3) == 2 and R.tracked(row, bad, nobs, 4) == 0


# ---- the replay against the sequential simulation ----------------------------------------------------------------------------------------------------
def build(scene):
    graph = MapGraph(**scene.graph())
    return graph, CullView(graph, **scene.view())


def replay_of_restated_tables(scene, lst, mono):
    t = R.tables(scene.world(), lst, mono)
    graph, view = build(scene)
    got = culling.keyframe_culling_replay(graph, view, lst, t["n_mps"], t["n_redundant"], t["row_offsets"], t["slot_count"], t["slot_flags"])
    return t, got


def assert_replay(scene, lst, mono):
    t, got = replay_of_restated_tables(scene, lst, mono)
    sim = R.keyframe_culling(scene.world(), lst, mono)
    keys = SEQUENCE_KEYS + ("mp_nobs", "mp_bad")
    assert subset(got, keys) == subset(sim, keys)
    return t, sim


@pytest.mark.parametrize("name", sorted(HAND_SCENES))
def test_replay_on_the_hand_scenes(name):
    make, exp = HAND_SCENES[name]
    scene, lst = make()
    _, sim = assert_replay(scene, lst, False)
    assert subset(sim, SEQUENCE_KEYS) == exp


@pytest.mark.parametrize("n", S.BOUNDARY_N)
def test_replay_on_the_09_boundary(n):
    for n_red in (n * 9 // 10, n * 9 // 10 + 1):
        assert_replay(*S.boundary(n, n_red), False)


def test_replay_monocular():
    assert_replay(*S.monocular_depths(), True)


# (n_kf, n_mp, max_obs, seed) of dense random graphs, chosen on the CPU so that in each of them the list order matters in both directions
ORDER_SEEDS = [(40, 300, 6, 32), (60, 300, 5, 76), (40, 300, 8, 4), (40, 300, 8, 59)]


@pytest.mark.parametrize("n_kf, n_mp, max_obs, seed", ORDER_SEEDS)
def test_replay_on_random_graphs_where_the_order_matters(n_kf, n_mp, max_obs, seed):
    scene = S.random_scene(seed, n_kf, n_mp, max_obs=max_obs, dense=True)
    lst = list(range(n_kf))
    t, sim = assert_replay(scene, lst, False)
    loses = [j for j in range(n_kf) if t["redundant"][j] and sim["decision"][j] == 0 and scene.mode[lst[j]] == 0]
    gains = [j for j in range(n_kf) if not t["redundant"][j] and sim["decision"][j] != 0]
    assert loses and gains, "a key frame redundant by the tables and kept, and one not redundant by the tables and culled"
    assert sim["went_bad"]


@pytest.mark.parametrize("dense", [False, True])
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("n_kf, n_mp", [(1, 5), (2, 40), (7, 120), (25, 300)])
def test_replay_on_random_graphs(n_kf, n_mp, seed, dense):
    scene = S.random_scene(100 * seed + n_kf, n_kf, n_mp, max_obs=6, dense=dense)
    assert_replay(scene, list(range(n_kf)), bool(seed & 1))
    assert_replay(scene, S.shuffled_list(seed, n_kf), bool(seed & 1))
    assert_replay(scene, [0, n_kf, -1, 0], False)                    # listed key frames outside the graph: an empty row, decision 0


# ---- the exports -------------------------------------------------------------------------------------------------------------------------------------------
def test_exports():
    import orb_line_slam_amd as ola
    for name in ("keyframe_culling_tables_batch", "KeyFrameCulling", "tracked_map_points_batch", "TrackedMapPoints", "map_point_culling", "MapPointCulling",
                 "keyframe_culling_replay"):
        assert name in ola.__all__ and callable(getattr(ola, name)), name
    assert "CullView" in ola.__all__ and ola.CullView is CullView


def test_no_new_status_bits():
    with open(os.path.join(ROOT, "orb_line_slam_amd", "csrc", "olf_internal.hpp")) as f:
        text = f.read()
    assert text.count("{STATUS_") == 7 and "STATUS_CONNECTIONS_LIST = 16384 };" in text      # the last bit and the last row are the ones that were there


def test_cull_view_checks_its_rows():
    scene, _ = S.octave_rule()
    graph = MapGraph(**scene.graph())
    for key, change in (("mp_obs_slot", lambda v: v[:-1]), ("kf_slot_octave", lambda v: [r + [0] for r in v]), ("mp_nobs", lambda v: v + [1]), ("kf_mode", lambda v: [3] * len(v)),
                        ("kf_slot_octave", lambda v: [[300] * len(r) for r in v]), ("kf_th_depth", lambda v: v[1:])):
        args = scene.view()
        args[key] = change(args[key])
        with pytest.raises(ValueError):
            CullView(graph, **args)


# ---- the C entries' argument checks (they come before the context is looked at) -------------------------------------------------------------------------
FAKE_CTX = C.c_void_p(1 << 20)                                       # not a context: a call that got past its argument checks would read it


def _args(a, dev):
    args = [v if not isinstance(v, np.ndarray) else _lib.ptr(v) for v in a.values()]
    return args + [None] if dev else args


def _scene_c():
    scene, _ = S.octave_rule()
    graph, view = build(scene)
    return graph, view


def _tables_call(graph_c, view_c, **change):
    i32, u8 = (lambda n: np.zeros(n, np.int32)), (lambda n: np.zeros(n, np.uint8))
    a = dict(ctx=FAKE_CTX, g=C.byref(graph_c), v=C.byref(view_c), n_list=2, kf_list=i32(2), mono=0, n_mps=i32(2), n_red=i32(2), red=u8(2), row=i32(3), cnt=i32(64),
             flags=u8(64), cap=64)
    a.update(change)
    return lib().olf_keyframe_culling_tables_dev(*_args(a, True))


def test_tables_bad_arguments_are_refused():
    graph, view = _scene_c()
    for change in (dict(ctx=None), dict(g=None), dict(v=None), dict(n_list=-1), dict(n_mps=None), dict(n_red=None), dict(red=None), dict(row=None), dict(cnt=None),
                   dict(flags=None), dict(cap=-1)):
        assert _tables_call(graph.c(), view.c(), **change) == OLF_ERR_INVALID and "olf_keyframe_culling_tables_dev" in last_error(), change
    for field in ("mp_obs_offsets", "mp_obs_kf", "mp_bad", "kf_mp_offsets", "kf_mp_index"):
        g = graph.c()
        setattr(g, field, None)
        assert _tables_call(g, view.c()) == OLF_ERR_INVALID, field
    for field in ("mp_obs_slot", "mp_nobs", "kf_slot_octave", "kf_slot_depth", "kf_th_depth"):
        v = view.c()
        setattr(v, field, None)
        assert _tables_call(graph.c(), v) == OLF_ERR_INVALID, field
    for field in ("n_kf", "n_mp"):
        g = graph.c()
        setattr(g, field, -1)
        assert _tables_call(g, view.c()) == OLF_ERR_INVALID, field


def _host_call(graph_c, view_c, **change):
    i32, u8 = (lambda n: np.zeros(n, np.int32)), (lambda n: np.zeros(n, np.uint8))
    a = dict(ctx=FAKE_CTX, g=C.byref(graph_c), v=C.byref(view_c), n_list=2, kf_list=i32(2), mono=0, decision=i32(2), n_mps=i32(2), n_red=i32(2), t_mps=i32(2), t_red=i32(2),
             t_flag=u8(2), nobs=i32(64), bad=u8(64), went=i32(64), n_went=i32(1))
    a.update(change)
    return lib().olf_keyframe_culling(*_args(a, False))


def test_host_form_bad_arguments_and_broken_offsets_are_refused():
    graph, view = _scene_c()
    for change in (dict(ctx=None), dict(g=None), dict(v=None), dict(n_list=-1), dict(decision=None), dict(n_mps=None), dict(n_red=None)):
        assert _host_call(graph.c(), view.c(), **change) == OLF_ERR_INVALID and "olf_keyframe_culling" in last_error(), change
    for field in ("mp_obs_slot", "mp_nobs", "kf_slot_octave", "kf_slot_depth", "kf_slot_stereo", "kf_th_depth", "kf_mode"):
        v = view.c()
        setattr(v, field, None)
        assert _host_call(graph.c(), v) == OLF_ERR_INVALID, field
    for field in ("mp_obs_offsets", "kf_mp_offsets"):
        graph, view = _scene_c()
        getattr(graph, field)[0] = 1
        assert _host_call(graph.c(), view.c()) == OLF_ERR_INVALID, field
        graph, view = _scene_c()
        getattr(graph, field)[2] = getattr(graph, field)[-1] + 1
        assert _host_call(graph.c(), view.c()) == OLF_ERR_INVALID, field


def _replay_call(graph_c, view_c, scene, lst, **change):
    t = R.tables(scene.world(), lst, False)
    i32 = lambda n: np.zeros(n, np.int32)
    n = len(lst)
    a = dict(g=C.byref(graph_c), v=C.byref(view_c), n_list=n, kf_list=np.asarray(lst, np.int32), t_mps=np.asarray(t["n_mps"], np.int32), t_red=np.asarray(t["n_redundant"], np.int32),
             row=np.asarray(t["row_offsets"], np.int32), cnt=np.asarray(t["slot_count"], np.int32), flags=np.asarray(t["slot_flags"], np.uint8), decision=i32(n), n_mps=i32(n),
             n_red=i32(n), nobs=None, bad=None, went=None, n_went=None)
    a.update(change)
    return lib().olf_keyframe_culling_replay(*_args(a, False))


def test_replay_bad_arguments_and_broken_offsets_are_refused():
    scene, lst = S.gains_redundancy("AB")
    graph, view = build(scene)
    assert _replay_call(graph.c(), view.c(), scene, lst) == 0        # the optional outputs may all be NULL
    for change in (dict(g=None), dict(v=None), dict(n_list=-1), dict(t_mps=None), dict(t_red=None), dict(row=None), dict(cnt=None), dict(flags=None), dict(decision=None),
                   dict(n_mps=None), dict(n_red=None)):
        assert _replay_call(graph.c(), view.c(), scene, lst, **change) == OLF_ERR_INVALID and "olf_keyframe_culling_replay" in last_error(), change
    for row in ([1, 11, 21], [0, 10, 21], [0, 11, 20], [0, 12, 11]):  # not the running sum of the listed rows' lengths (11 and 10)
        assert _replay_call(graph.c(), view.c(), scene, lst, row=np.asarray(row, np.int32)) == OLF_ERR_INVALID, row
    for field in ("mp_obs_offsets", "kf_mp_offsets"):
        graph, view = build(scene)
        getattr(graph, field)[2] = getattr(graph, field)[-1] + 1
        assert _replay_call(graph.c(), view.c(), scene, lst) == OLF_ERR_INVALID, field
    for field in ("mp_obs_slot", "mp_nobs", "kf_slot_octave", "kf_slot_stereo", "kf_mode"):
        graph, view = build(scene)
        v = view.c()
        setattr(v, field, None)
        assert _replay_call(graph.c(), v, scene, lst) == OLF_ERR_INVALID, field


@pytest.mark.parametrize("name", ["olf_tracked_map_points", "olf_tracked_map_points_batch_dev"])
def test_tracked_bad_arguments_are_refused(name):
    scene = S.with_lines(S.random_scene(3, 4, 20))
    graph = MapGraph(**scene.graph())
    i32 = lambda n: np.zeros(n, np.int32)

    def call(graph_c, **change):
        a = dict(ctx=FAKE_CTX, g=C.byref(graph_c), mp_nobs=i32(20), ml_nobs=i32(20), n_list=2, kf_list=i32(2), min_p=1, min_l=1, n_points=i32(2), n_lines=i32(2))
        a.update(change)
        return getattr(lib(), name)(*_args(a, name.endswith("_dev")))

    for change in (dict(ctx=None), dict(g=None), dict(n_list=-1), dict(n_points=None), dict(n_lines=None), dict(mp_nobs=None), dict(ml_nobs=None)):
        assert call(graph.c(), **change) == OLF_ERR_INVALID and name in last_error(), change
    for field in ("kf_mp_offsets", "mp_bad", "ml_bad"):
        g = graph.c()
        setattr(g, field, None)
        assert call(g) == OLF_ERR_INVALID, field
    for field in ("n_kf", "n_mp", "n_ml"):
        g = graph.c()
        setattr(g, field, -1)
        assert call(g) == OLF_ERR_INVALID, field
    if not name.endswith("_dev"):
        for field in ("kf_mp_offsets", "kf_ml_offsets"):
            graph = MapGraph(**scene.graph())
            getattr(graph, field)[0] = 1
            assert call(graph.c()) == OLF_ERR_INVALID, field
            graph = MapGraph(**scene.graph())
            getattr(graph, field)[2] = getattr(graph, field)[-1] + 1
            assert call(graph.c()) == OLF_ERR_INVALID, field


@pytest.mark.parametrize("name", ["olf_map_point_culling", "olf_map_point_culling_dev"])
def test_map_point_culling_bad_arguments_are_refused(name):
    a = S.recent_points(0, 12)

    def call(**change):
        args = dict(ctx=FAKE_CTX, n=12, bad=a["bad"], found=a["found"], visible=a["visible"], nobs=a["nobs"], first=a["first_kf_id"], cur=C.c_int64(10), mono=0,
                    action=np.zeros(12, np.uint8))
        args.update(change)
        return getattr(lib(), name)(*_args(args, name.endswith("_dev")))

    for change in (dict(ctx=None), dict(n=-1), dict(bad=None), dict(found=None), dict(visible=None), dict(nobs=None), dict(first=None), dict(action=None)):
        assert call(**change) == OLF_ERR_INVALID and name in last_error(), change


# ---- the reference-side adaptor ----------------------------------------------------------------------------------------------------------------------------
def build_adaptor(exe):
    libdir = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "adaptor_culling.cpp"), "-L" + libdir, "-lorbline_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_adaptor_replay_path(tmp_path):
    """compiled with -Wall -Werror, linked, and run without a device: the snapshot, the view, olf_keyframe_culling_replay on hand-worked tables and
    ApplyKeyFrameCulling on objects whose SetBadFlag is the reference's.  KeyFrameCulling itself (the host form) runs in tests/test_culling_gpu.py."""
    exe = str(tmp_path / "adaptor_culling")
    build_adaptor(exe)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert out.returncode == 0 and b"ADAPTOR_CULLING_OK" in out.stdout, out.stdout.decode()[-3000:]
