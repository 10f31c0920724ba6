"""KeyFrame::UpdateConnections without a device: the restatement (tests/connections_reference.py) against answers worked out by hand from
src/KeyFrame.cc:446-557 and printed beside the scenes (tests/connections_scenes.py), the argument checks of the three C entries, the constants the layers
share, and the reference-side adaptor (ApplyConnections: include/orbline_reference_api.hpp) compiled against stand-in types and run."""
import ctypes as C
import inspect
import os
import subprocess
import numpy as np
import pytest
import connections_reference as R
import connections_scenes as S
from orb_line_slam_amd import MapGraph, _lib, connections
from orb_line_slam_amd._lib import OLF_ERR_INVALID, last_error, lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against hand-worked answers -----------------------------------------------------------------------------------------------------
def test_equal_weights_order_descending_index_and_the_maximum_is_the_lowest():
    """weights 20, 20, 16: the row is [higher index, lower index, third], pKFmax the lower index"""
    assert R.update_connections(S.three_weights().graph(), 0) == S.THREE_WEIGHTS_EXPECTED


def test_all_below_th_leaves_one_pair():
    assert R.update_connections(S.all_below_th().graph(), 2) == S.ALL_BELOW_TH_EXPECTED


def test_counts_around_th():
    assert R.update_connections(S.around_th().graph(), 0, th=15) == S.AROUND_TH_EXPECTED
    assert R.update_connections(S.around_th().graph(), 0, th=16)["ordered"] == [3] and R.update_connections(S.around_th().graph(), 0, th=14)["ordered"] == [3, 2, 1]


def test_slot_rules():
    """a self-observation, a bad point, a NULL slot, a point in two slots"""
    assert R.update_connections(S.slot_rules().graph(), 1, th=1) == S.SLOT_RULES_EXPECTED


@pytest.mark.parametrize("scene, th", [(S.slot_rules, 1), (S.three_weights, 15), (lambda: S.random_graph(5, 30, 200), 3)])
def test_lines_do_not_vote(scene, th):
    plain, lines = scene(), S.with_lines(scene())
    assert lines.kf_ml is not None and any(lines.kf_ml)
    assert R.update_connections_list(plain.graph(), None, th) == R.update_connections_list(lines.graph(), None, th)


def test_empty_cases():
    out = R.update_connections_list(S.empties().graph(), None, 1)
    for k in range(4):
        assert out[k] == dict(connected=[], weights=[], ordered=[], ordered_weights=[], kf_max=-1, w_max=0, n_counted=0), k
    assert out[4]["connected"] == [1] and out[4]["ordered"] == [1]


def test_best_covisibles_restatement():
    assert R.update_best_covisibles({4: 2, 1: 9, 7: 2, 3: 9, 0: 1}) == ([3, 1, 7, 4, 0], [9, 9, 2, 2, 1])
    assert R.update_best_covisibles({}) == ([], [])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_survivor_scenes_reach_their_count(n):
    s = S.survivors(n)
    out = R.update_connections(s.graph(), min(3, n), th=1)
    assert out["n_counted"] == n and len(out["ordered"]) == n and len(set(out["ordered_weights"])) == min(n, 5)


# ---- the constants the layers share ------------------------------------------------------------------------------------------------------------------------
def test_th_default_is_the_headers():
    with open(os.path.join(ROOT, "include", "orbline.h")) as f:
        assert "#define OLF_COVIS_TH 15 " in f.read()
    assert connections.OLF_COVIS_TH == 15
    for f in (connections.UpdateConnections, connections.update_connections_batch):
        assert inspect.signature(f).parameters["th"].default == 15


def test_status_text_of_the_new_bit():
    """the list bit names the entries that own the lists, as bit 8192 does; the rows before it are untouched"""
    with open(os.path.join(ROOT, "orb_line_slam_amd", "csrc", "olf_internal.hpp")) as f:
        text = f.read()
    assert 'STATUS_CONNECTIONS_LIST = 16384' in text
    assert '{STATUS_CONNECTIONS_LIST, "connected or ordered key-frame list of olf_update_connections_batch_dev, or a row of olf_best_covisibles_batch_dev"}' in text
    assert text.index('{STATUS_LOCALMAP_LIST, "local key-frame, map-point or map-line list of olf_update_local_map_batch_dev"}') < text.index("{STATUS_CONNECTIONS_LIST,")


def test_exports():
    import orb_line_slam_amd as ola
    for name in ("UpdateConnections", "update_connections_batch", "best_covisibles_batch"):
        assert name in ola.__all__ and callable(getattr(ola, name))


# ---- the C entries' argument checks (they come before the context is looked at) -------------------------------------------------------------------------
def _call(name, graph_c, **change):
    """the entry `name` on a graph and two listed key frames' worth of buffers, with the named arguments NULL / changed"""
    i32 = lambda n: np.zeros(n, np.int32)
    a = dict(ctx=C.c_void_p(1 << 20), g=C.byref(graph_c), n_list=2, kf_list=i32(2), th=15, nc=i32(2), kmax=i32(2), wmax=i32(2), conn_off=i32(3), conn_idx=i32(4),
             conn_w=i32(4), conn_cap=4, cov_off=i32(3), cov_idx=i32(4), cov_w=i32(4), cov_cap=4)
    a.update(change)
    args = [v if not isinstance(v, np.ndarray) else _lib.ptr(v) for v in a.values()]
    if name.endswith("_dev"):
        args.append(None)
    return getattr(lib(), name)(*args)


@pytest.mark.parametrize("name", ["olf_update_connections", "olf_update_connections_batch_dev"])
def test_bad_arguments_are_refused(name):
    """the context handed over is not one: a call that got past its argument checks would read it"""
    graph = MapGraph(**S.slot_rules().graph())
    for change in (dict(ctx=None), dict(g=None), dict(n_list=-1), dict(th=0), dict(th=-3), dict(nc=None), dict(kmax=None), dict(wmax=None), dict(conn_off=None),
                   dict(cov_off=None), dict(conn_idx=None), dict(conn_w=None), dict(cov_idx=None), dict(cov_w=None), dict(conn_cap=-1), dict(cov_cap=-1)):
        assert _call(name, graph.c(), **change) == OLF_ERR_INVALID and name in last_error(), change
    for field in ("mp_obs_offsets", "mp_bad", "kf_mp_offsets"):
        g = graph.c()
        setattr(g, field, None)
        assert _call(name, g) == OLF_ERR_INVALID, field
    for field in ("n_kf", "n_mp"):
        g = graph.c()
        setattr(g, field, -1)
        assert _call(name, g) == OLF_ERR_INVALID, field


def test_host_form_checks_the_offsets_it_reads_and_no_others():
    for field in ("mp_obs_offsets", "kf_mp_offsets"):
        graph = MapGraph(**S.slot_rules().graph())
        getattr(graph, field)[0] = 1
        assert _call("olf_update_connections", graph.c()) == OLF_ERR_INVALID, field
        graph = MapGraph(**S.slot_rules().graph())
        getattr(graph, field)[2] = getattr(graph, field)[-1] + 1
        assert _call("olf_update_connections", graph.c()) == OLF_ERR_INVALID, field


def test_best_covisibles_bad_arguments_are_refused():
    i32 = lambda n: np.zeros(n, np.int32)
    base = dict(ctx=C.c_void_p(1 << 20), n_rows=2, off=i32(3), idx=i32(4), w=i32(4), out_idx=i32(4), out_w=i32(4))
    for change in (dict(ctx=None), dict(n_rows=-1), dict(off=None), dict(idx=None), dict(w=None), dict(out_idx=None), dict(out_w=None)):
        a = dict(base)
        a.update(change)
        args = [v if not isinstance(v, np.ndarray) else _lib.ptr(v) for v in a.values()] + [None]
        assert lib().olf_best_covisibles_batch_dev(*args) == OLF_ERR_INVALID and "olf_best_covisibles_batch_dev" in last_error(), change


# ---- the reference-side adaptor ----------------------------------------------------------------------------------------------------------------------------
def build_adaptor(exe):
    libdir = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "adaptor_connections.cpp"), "-L" + libdir, "-lorbline_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)


def test_adaptor_apply_connections(tmp_path):
    """compiled with -Wall -Werror, linked, and run without a device: ApplyConnections on the hand-worked outputs.  UpdateConnections itself (the host form)
    runs in tests/test_connections_gpu.py."""
    exe = str(tmp_path / "adaptor_connections")
    build_adaptor(exe)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
    assert out.returncode == 0 and b"ADAPTOR_CONNECTIONS_OK" in out.stdout, out.stdout.decode()[-3000:]
