"""Tracking::UpdateLocalMap without a device: the restatement (tests/localmap_reference.py) against answers worked out on paper from
src/Tracking.cc:2039-2205, the argument checks of orb_line_slam_amd.MapGraph and of the two C entries, and the reference-side adaptor
(MapGraphOf, WriteBack: include/orbline_reference_api.hpp) compiled against stand-in types and run."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import localmap_reference as R
import localmap_scenes as S
from orb_line_slam_amd import MapGraph, _lib
from orb_line_slam_amd._lib import OLF_ERR_INVALID, last_error, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(scene):
    return R.Map(**scene.graph()).update_local_map(scene.frame_mp, scene.frame_ml)


# ---- the restatement against hand-worked answers -----------------------------------------------------------------------------------------------------
def test_five_key_frames_by_hand():
    """the derivation stands beside FIVE_KF_EXPECTED in tests/localmap_scenes.py"""
    assert run(S.five_kf()) == S.FIVE_KF_EXPECTED


@pytest.mark.parametrize("n_equal", [2, 3])
def test_lowest_index_wins_a_tie(n_equal):
    """`it->second > max` is strict and the std::map iterates in ascending address = index (C.16): of the key frames 3, 5[, 6] with 4 votes each, 3"""
    (got,) = run(S.ties(n_equal))
    assert got["ref_kf"] == 3 and got["n_voted"] == 3 + n_equal - 1 and got["local_kfs"] == sorted(got["local_kfs"])


def test_bad_key_frame_with_most_votes_is_neither_listed_nor_the_reference():
    """:2134: `continue` comes before the comparison, so 2 (5 votes, bad) is skipped and 4 (3 votes) is pKFmax; 2 still counts in keyframeCounter"""
    (got,) = run(S.bad_kf_has_most_votes())
    assert got["ref_kf"] == 4 and got["n_voted"] == 3 and got["local_kfs"] == [1, 4]


def test_only_ten_neighbours_are_read():
    (got,) = run(S.eleventh_neighbour_free())
    assert got["local_kfs"] == [0, 1, 2, 3, 4, 5]


def test_children_are_visited_in_ascending_index():
    """children of 2: 1 (bad), 3, 4 (stamped), 5 -> 3; then member 4 has nothing to add"""
    (got,) = run(S.child_after_bad_child())
    assert got["local_kfs"] == [2, 4, 3]


def test_parent_is_not_tested_for_bad():
    (got,) = run(S.bad_parent())
    assert got["local_kfs"] == [2, 0]


def test_parent_ends_the_loop():
    (got,) = run(S.parent_at_first_member())
    assert got["local_kfs"] == [1, 2, 3, 0]


@pytest.mark.parametrize("n_first, n_added", [(79, 2), (80, 1), (81, 0)])
def test_the_loop_stops_once_the_list_holds_more_than_80(n_first, n_added):
    """`size() > 80` is tested before a member is visited: a list of 79 grows to 81 over two members, one of 80 over one, one of 81 not at all"""
    (got,) = run(S.first_list_of(n_first))
    assert got["local_kfs"][:n_first] == list(range(10, 10 + n_first)) and len(got["local_kfs"]) == n_first + n_added


def test_first_occurrence_wins_by_position():
    s = S.dup_in_one_kf()
    (got,) = run(s)
    slots = s.kf_mp[0]
    assert slots[3] == slots[7] and got["local_points"] == slots[:7] + slots[8:]
    s = S.dup_across_two_kfs()
    (got,) = run(s)
    seen, want = set(), []
    for v in s.kf_mp[0] + s.kf_mp[1]:
        if v not in seen:
            seen.add(v); want.append(v)
    assert got["local_kfs"] == [0, 1] and got["local_points"] == want and len(want) < len(s.kf_mp[0] + s.kf_mp[1]) - 2


def test_empty_cases():
    a, b, c = run(S.frame_holds_nothing())
    for got, n in ((a, 3), (c, 0)):
        assert got["n_voted"] == 0 and got["ref_kf"] == -1 and got["local_kfs"] == got["local_points"] == got["local_lines"] == [] and len(got["frame_mp"]) == n
    assert b["n_voted"] == 1 and b["local_kfs"] == [1]
    (got,) = run(S.all_voted_bad())
    assert got["n_voted"] == 2 and got["ref_kf"] == -1 and got["local_kfs"] == got["local_points"] == []


def test_random_scenes_have_what_they_are_for():
    """the random graphs of the GPU test reach the extension loop, drop bad points and meet duplicates"""
    s = S.random_scene(3, 65, 300, 17, n_ml=100)
    out = run(s)
    assert any(len(o["local_kfs"]) > o["n_voted"] for o in out) and any(0 < len(o["local_kfs"]) < o["n_voted"] for o in out)
    assert any(-1 in o["frame_mp"] and any(v >= 0 for v in o["frame_mp"]) for o in out)
    assert any(len(o["local_points"]) > 50 for o in out) and any(len(o["local_lines"]) > 10 for o in out)
    assert any(len(r) != len(set(r)) for r in s.kf_mp)


# ---- MapGraph ----------------------------------------------------------------------------------------------------------------------------------------------
def test_map_graph_arrays():
    s = S.five_kf()
    g = MapGraph(**s.graph())
    assert (g.n_kf, g.n_mp, g.n_ml) == (5, 6, 3)
    assert g.kf_mp_offsets.tolist() == [0, 2, 5, 7, 9, 11] and g.kf_mp_index.tolist() == [5, 0, 0, -1, 2, 4, 3, 1, 0, 3, 2]
    assert g.kf_child_offsets.tolist() == [0, 1, 4, 4, 4, 4] and g.kf_child_index.tolist() == [1, 2, 3, 4]        # (given as 4, 2, 3: sorted, C.16)
    assert g.kf_parent.tolist() == [-1, 0, 1, 1, 1] and g.mp_bad.dtype == np.uint8 and g.kf_covis_index.dtype == np.int32
    c = g.c()
    assert c.n_kf == 5 and c.kf_ml_offsets and c.ml_bad
    g = MapGraph(**S.voting(3, {1: 1}).graph())
    assert g.n_ml == 0 and g.c().kf_ml_offsets is None and g.c().ml_bad is None


@pytest.mark.parametrize("change, message", [
    (lambda a: a["mp_obs"][0].append(5), "mp_obs: a key-frame index outside"),
    (lambda a: a["kf_covis"][1].append(-1), "kf_covis: a key-frame index outside"),
    (lambda a: a["kf_children"][0].append(9), "kf_children: a key-frame index outside"),
    (lambda a: a["kf_children"][1].append(2), "lists a child twice"),
    (lambda a: a["kf_parent"].__setitem__(2, -2), "kf_parent: a key-frame index outside"),
    (lambda a: a["kf_mp"][0].append(6), "kf_mp: a map-point index outside"),
    (lambda a: a["kf_ml"][0].append(3), "kf_ml: a map-line index outside"),
    (lambda a: a["kf_mp"].pop(), "kf_mp: 5 rows expected"),
    (lambda a: a["mp_bad"].append(0), "mp_obs: 7 rows expected"),
    (lambda a: a.__setitem__("ml_bad", None), "come together"),
    (lambda a: a["kf_parent"].pop(), "kf_parent: 5 entries expected"),
])
def test_map_graph_refuses(change, message):
    a = S.five_kf().graph()
    change(a)
    with pytest.raises(ValueError, match=message):
        MapGraph(**a)


def test_map_graph_refuses_more_key_frames_than_the_vote_table_holds():
    from orb_line_slam_amd.localmap import OLF_LOCALMAP_MAX_KF
    assert OLF_LOCALMAP_MAX_KF >= 8192
    s = S.Scene(OLF_LOCALMAP_MAX_KF + 1)
    with pytest.raises(ValueError, match="OLF_LOCALMAP_MAX_KF"):
        MapGraph(**s.graph())
    with open(os.path.join(ROOT, "include", "orbline.h")) as f:
        assert "#define OLF_LOCALMAP_MAX_KF %d\n" % OLF_LOCALMAP_MAX_KF in f.read()


# ---- the C entries' argument checks (they come before the context is looked at) -------------------------------------------------------------------------
def _call(name, graph_c, **null):
    """the entry `name` on a graph and one frame's worth of buffers, with the named arguments NULL / changed"""
    i32 = lambda n: np.zeros(n, np.int32)
    a = dict(ctx=C.c_void_p(1 << 20), g=C.byref(graph_c), n_frames=1, img_stride=1, counts=i32(1), lcounts=i32(1), frame_mp=i32(8), frame_ml=None, mp_out=None,
             ml_out=None, ref=i32(1), nv=i32(1), kf_off=i32(2), kf_idx=i32(4), kf_cap=4, mp_off=i32(2), mp_idx=i32(4), mp_cap=4, ml_off=i32(2), ml_idx=i32(4), ml_cap=4)
    a.update(null)
    args = [v if not isinstance(v, np.ndarray) else _lib.ptr(v) for v in a.values()]
    if name.endswith("_dev"):
        args.append(None)
    return getattr(lib(), name)(*args)


@pytest.mark.parametrize("name", ["olf_update_local_map", "olf_update_local_map_batch_dev"])
def test_bad_arguments_are_refused(name):
    """the context handed over is not one: a call that got past its argument checks would read it"""
    graph = MapGraph(**S.five_kf().graph())
    for null in (dict(ctx=None), dict(g=None), dict(n_frames=-1), dict(img_stride=0), dict(frame_mp=None), dict(ref=None), dict(nv=None), dict(kf_off=None),
                 dict(mp_off=None), dict(ml_off=None), dict(kf_idx=None), dict(mp_idx=None), dict(ml_idx=None), dict(kf_cap=-1), dict(mp_cap=-1), dict(ml_cap=-1)):
        assert _call(name, graph.c(), **null) == OLF_ERR_INVALID and name in last_error(), null
    for field in ("kf_bad", "kf_mp_offsets", "kf_covis_offsets", "kf_child_offsets", "kf_parent", "mp_obs_offsets", "mp_bad", "ml_bad", "kf_ml_offsets"):
        g = graph.c()
        setattr(g, field, None)
        assert _call(name, g) == OLF_ERR_INVALID, field
    g = graph.c()
    g.n_kf = -1
    assert _call(name, g) == OLF_ERR_INVALID


def test_host_form_checks_the_graph():
    """offsets that do not start at 0 or decrease, and children that do not ascend strictly (C.16), are OLF_ERR_INVALID before anything is uploaded"""
    graph = MapGraph(**S.five_kf().graph())
    graph.kf_child_index[1:3] = [3, 2]
    assert _call("olf_update_local_map", graph.c()) == OLF_ERR_INVALID and "ascend" in last_error()
    graph.kf_child_index[1:3] = [2, 2]
    assert _call("olf_update_local_map", graph.c()) == OLF_ERR_INVALID and "ascend" in last_error()
    for field in ("mp_obs_offsets", "kf_mp_offsets", "kf_ml_offsets", "kf_covis_offsets", "kf_child_offsets"):
        graph = MapGraph(**S.five_kf().graph())
        getattr(graph, field)[0] = 1
        assert _call("olf_update_local_map", graph.c()) == OLF_ERR_INVALID, field
        graph = MapGraph(**S.five_kf().graph())
        getattr(graph, field)[2] = getattr(graph, field)[-1] + 1
        assert _call("olf_update_local_map", graph.c()) == OLF_ERR_INVALID, field


def test_status_text_of_the_new_bits():
    """bit 4096's description is general (it names no entry point); the list bit names the one entry that owns the lists, as bit 128 does"""
    with open(os.path.join(ROOT, "orb_line_slam_amd", "csrc", "olf_internal.hpp")) as f:
        text = f.read()
    assert 'STATUS_KF_INDEX = 4096' in text and '{STATUS_KF_INDEX, "a map-graph entry left out a key-frame index outside the graph"}' in text
    assert 'STATUS_LOCALMAP_LIST = 8192' in text


# ---- the reference-side adaptor ----------------------------------------------------------------------------------------------------------------------------
def test_adaptor_map_graph_and_write_back(tmp_path):
    exe = str(tmp_path / "adaptor_localmap")
    libdir = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "adaptor_localmap.cpp"), "-L" + libdir, "-lorbline_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert out.returncode == 0 and b"ADAPTOR_LOCALMAP_OK" in out.stdout, out.stdout.decode()[-3000:]
