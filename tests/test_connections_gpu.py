"""GPU parity: olf_update_connections_batch_dev, olf_update_connections and olf_best_covisibles_batch_dev -- KeyFrame::UpdateConnections
(src/KeyFrame.cc:446-557) for a list of key frames against one snapshot of the map, and KeyFrame::UpdateBestCovisibles (:216-235) for a batch of rows.  Every
comparison is exact equality of every output with the line-by-line restatement (tests/connections_reference.py); the scenes (tests/connections_scenes.py)
are the smallest at which each rule can go wrong.  The context is 320 x 240, the smallest image the batch tests use."""
import ctypes as C
import subprocess
import numpy as np
import pytest
import connections_reference as R
import connections_scenes as S
import localmap_reference as LR
import orb_line_slam_amd as ola
from orb_line_slam_amd import MapGraph, _lib, connections, localmap
from orb_line_slam_amd._lib import OLF_ERR_CAPACITY, OlfError, lib

pytestmark = pytest.mark.gpu

STATUS_TEXT = {
    512: "a batched point entry left out a list index or a per-frame map-point index outside the map",
    4096: "a map-graph entry left out a key-frame index outside the graph",
    16384: "connected or ordered key-frame list of olf_update_connections_batch_dev, or a row of olf_best_covisibles_batch_dev",
}
SENTINEL = -7
EMPTY = dict(connected=[], weights=[], ordered=[], ordered_weights=[], kf_max=-1, w_max=0, n_counted=0)


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


def totals(exp):
    return [sum(len(e["connected"]) for e in exp), sum(len(e["ordered"]) for e in exp)]


def run_dev(ctx, graph, kf_list, n_list, th, capacities, slack=8):
    """the device form; returns a dict of numpy arrays.  The index and weight tensors are `slack` longer than the capacity told, every output is filled with
    SENTINEL: nothing may be written past a list or a capacity."""
    import torch
    full = lambda n: torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")
    out = {}
    for k, c in zip(("conn", "covis"), capacities):
        out[k + "_offsets"], out[k + "_index"], out[k + "_weight"] = full(n_list + 1), full(c + slack), full(c + slack)
    for k in ("n_counted", "kf_max", "w_max"):
        out[k] = full(max(n_list, 1))
    res = connections.update_connections_batch(graph, None if kf_list is None else up(np.asarray(kf_list, np.int32)), n_list=n_list, th=th, capacities=capacities,
                                               out=out, context=ctx)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in res.items()}
    got["capacities"] = list(capacities)
    return got


def assert_equal(got, exp, truncated=False):
    """every output of the device form against the restatement's per-key-frame answers"""
    n = len(exp)
    for k, key, wkey, cap in (("conn", "connected", "weights", got["capacities"][0]), ("covis", "ordered", "ordered_weights", got["capacities"][1])):
        want = np.concatenate([[0], np.cumsum([len(e[key]) for e in exp])])
        assert np.array_equal(got[k + "_offsets"], want), (k, got[k + "_offsets"], want)
        for name, field in ((k + "_index", key), (k + "_weight", wkey)):
            flat = np.asarray([v for e in exp for v in e[field]], np.int32)
            assert truncated or len(flat) <= cap
            m = min(len(flat), cap)
            assert np.array_equal(got[name][:m], flat[:m]), name
            assert np.all(got[name][m:] == SENTINEL), name + ": written past the list or the capacity"
    for k in ("n_counted", "kf_max", "w_max"):
        assert [int(v) for v in got[k][:n]] == [e[k] for e in exp], k


def check(ctx, scene, kf_list=None, th=15, graph=None, exp=None):
    exp = R.update_connections_list(scene.graph(), kf_list, th) if exp is None else exp
    graph = MapGraph(**scene.graph()) if graph is None else graph
    got = run_dev(ctx, graph, kf_list, len(exp), th, totals(exp))
    assert_equal(got, exp)
    ctx.poll_status()
    return exp, got, graph


# ---- 1: random graphs ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th", [1, 3, 15])
@pytest.mark.parametrize("n_mp", [0, 40, 300])
@pytest.mark.parametrize("n_kf", [1, 2, 7, 65, 300])
def test_random_graphs(ctx, n_kf, n_mp, th):
    scene = S.random_graph(1000 * n_kf + n_mp, n_kf, n_mp, max_obs=40 if n_mp == 300 else 12)
    exp, _, graph = check(ctx, scene, None, th)
    lst = S.shuffled_list(n_kf + n_mp, n_kf)
    assert lst != sorted(lst) or n_kf <= 2
    assert len(set(lst)) < len(lst)
    check(ctx, scene, lst, th, graph=graph)
    if n_mp == 300 and (n_kf, th) in ((65, 15), (300, 3)):           # the threshold keeps a part of KFcounter ...
        assert any(1 < len(e["ordered"]) < e["n_counted"] for e in exp)
    if n_mp == 300 and (n_kf, th) == (300, 15):                      # ... or nothing, and the fallback pair stands in
        assert any(len(e["ordered"]) == 1 and e["ordered_weights"][0] < 15 and e["n_counted"] > 1 for e in exp)


# ---- 2: sizes of the ordered row: the sort's padding, more than one pass of the workgroup ------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1000])
def test_survivor_counts(ctx, n):
    scene = S.survivors(n)
    kf = min(3, n)
    exp, _, _ = check(ctx, scene, [kf], 1)
    assert exp[0]["n_counted"] == n and len(exp[0]["ordered"]) == n


# ---- 3: ties ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 70])
def test_ties(ctx, n):
    """n key frames of weight 3 around key frame 1 and one of weight 1: descending index in the row, the lowest index is pKFmax"""
    scene = S.equal_weights(n)
    exp, _, _ = check(ctx, scene, [1], 1)
    tied = [k for k in range(n + 1) if k != 1]
    assert exp[0]["ordered"] == tied[::-1] + [n + 1] and exp[0]["kf_max"] == 0 and exp[0]["w_max"] == 3
    exp, _, _ = check(ctx, scene, [1], 3)
    assert exp[0]["ordered"] == tied[::-1] and exp[0]["connected"] == tied + [n + 1]


# ---- 4: the fallback pair and the threshold's boundary --------------------------------------------------------------------------------------------------
def test_fallback_pair(ctx):
    exp, _, _ = check(ctx, S.all_below_th(), [2], 15)
    assert exp[0] == S.ALL_BELOW_TH_EXPECTED


def test_around_th(ctx):
    exp, _, _ = check(ctx, S.around_th(), [0], 15)
    assert exp[0] == S.AROUND_TH_EXPECTED
    check(ctx, S.around_th(), None, 15)
    check(ctx, S.around_th(), None, 16)
    check(ctx, S.around_th(), None, 14)


def test_hand_worked_scenes(ctx):
    exp, _, _ = check(ctx, S.three_weights(), [0], 15)
    assert exp[0] == S.THREE_WEIGHTS_EXPECTED
    exp, _, _ = check(ctx, S.slot_rules(), [1], 1)
    assert exp[0] == S.SLOT_RULES_EXPECTED


def test_lines_are_not_read(ctx):
    """a graph with and without kf_ml_* gives the same result"""
    plain, lines = S.random_graph(5, 30, 200), S.with_lines(S.random_graph(5, 30, 200))
    exp, _, _ = check(ctx, plain, None, 3)
    _, _, graph = check(ctx, lines, None, 3, exp=exp)
    assert graph.n_ml > 0 and graph.c_dev().kf_ml_offsets


# ---- 5: weights and table ends ------------------------------------------------------------------------------------------------------------------------------
def test_weight_beyond_16_bits(ctx):
    scene = S.one_point_in_many_slots(70000)
    exp, _, _ = check(ctx, scene, None, 15)
    assert exp[0]["weights"] == [70000] and exp[0]["ordered_weights"] == [70000] and exp[1]["weights"] == [1]


def test_first_and_last_key_frame_of_the_table(ctx):
    n = localmap.OLF_LOCALMAP_MAX_KF
    scene = S.table_ends(n, 100)
    exp, _, _ = check(ctx, scene, [100, 0, n - 1], 1)
    assert exp[0]["connected"] == [0, n - 1] and exp[0]["weights"] == [2, 3] and exp[0]["ordered"] == [n - 1, 0]
    assert exp[2]["connected"] == [0, 100] and exp[2]["ordered"] == [100, 0]


def test_too_many_key_frames_are_refused_before_any_launch(ctx):
    import torch
    n = localmap.OLF_LOCALMAP_MAX_KF + 1
    g = _lib.MapGraphC()
    z = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    g.n_kf, g.n_mp, g.n_ml = n, 0, 0
    g.mp_obs_offsets = g.kf_mp_offsets = z.data_ptr()
    out = torch.full((8,), SENTINEL, dtype=torch.int32, device="cuda")
    p = out.data_ptr()
    rc = lib().olf_update_connections_batch_dev(ctx.handle, C.byref(g), 1, None, 15, p, p, p, p, p, p, 4, p, p, p, 4, None)
    assert rc == OLF_ERR_CAPACITY and "OLF_LOCALMAP_MAX_KF" in _lib.last_error()
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy() == SENTINEL)
    ctx.poll_status()


# ---- 6: empty cases --------------------------------------------------------------------------------------------------------------------------------------
def test_empty_cases(ctx):
    """no slots; only bad points; only self-observations; only NULL slots"""
    exp, got, _ = check(ctx, S.empties(), None, 1)
    assert exp[:4] == [EMPTY] * 4 and exp[4]["n_counted"] == 1
    assert got["kf_max"][:4].tolist() == [-1] * 4


def test_no_list_writes_nothing(ctx):
    scene = S.three_weights()
    got = run_dev(ctx, MapGraph(**scene.graph()), None, 0, 15, [4, 4])
    for k in ("conn_offsets", "covis_offsets", "conn_index", "conn_weight", "covis_index", "covis_weight", "n_counted", "kf_max", "w_max"):
        assert np.all(got[k] == SENTINEL), k
    ctx.poll_status()
    assert ola.UpdateConnections(MapGraph(**scene.graph()), [], context=ctx) == []


# ---- 7: malformed indices -----------------------------------------------------------------------------------------------------------------------------
def _status(ctx, bit):
    with pytest.raises(OlfError) as e:
        ctx.poll_status()
    assert e.value.code == OLF_ERR_CAPACITY and "flags=%d (%d: %s)" % (bit, bit, STATUS_TEXT[bit]) in str(e.value), str(e.value)
    ctx.poll_status()                                                # (read and cleared)


def _malformed_base():
    scene = S.random_graph(77, 30, 200)
    exp = R.update_connections_list(scene.graph(), None, 3)
    kf = next(k for k, e in enumerate(exp) if len(e["ordered"]) > 2)
    return scene, kf


def test_malformed_slot_index(ctx):
    scene, kf = _malformed_base()
    graph = MapGraph(**scene.graph())
    slot = next(i for i, v in enumerate(scene.kf_mp[kf]) if v >= 0 and not scene.mp_bad[v] and len(scene.mp_obs[v]) > 1)
    graph.kf_mp_index[graph.kf_mp_offsets[kf] + slot] = graph.n_mp + 5
    scene.kf_mp[kf][slot] = -1                                        # left out = as if the slot were NULL
    exp = R.update_connections_list(scene.graph(), None, 3)
    assert_equal(run_dev(ctx, graph, None, len(exp), 3, totals(exp)), exp)
    _status(ctx, 512)


@pytest.mark.parametrize("value", ["n_kf", -3])
def test_malformed_observation(ctx, value):
    scene, kf = _malformed_base()
    graph = MapGraph(**scene.graph())
    p = next(v for v in scene.kf_mp[kf] if v >= 0 and not scene.mp_bad[v] and len(scene.mp_obs[v]) > 1)
    at = next(i for i, o in enumerate(scene.mp_obs[p]) if o != kf)
    graph.mp_obs_kf[graph.mp_obs_offsets[p] + at] = graph.n_kf if value == "n_kf" else value
    before = R.update_connections(scene.graph(), kf, 3)
    scene.mp_obs[p] = scene.mp_obs[p][:at] + scene.mp_obs[p][at + 1:]
    exp = R.update_connections_list(scene.graph(), None, 3)
    assert exp[kf] != before
    assert_equal(run_dev(ctx, graph, None, len(exp), 3, totals(exp)), exp)
    _status(ctx, 4096)


def test_listed_key_frame_outside_the_graph(ctx):
    scene, kf = _malformed_base()
    graph = MapGraph(**scene.graph())
    lst = [kf, graph.n_kf, 2, -1, kf]
    exp = [R.update_connections(scene.graph(), k, 3) if 0 <= k < graph.n_kf else dict(EMPTY) for k in lst]
    assert_equal(run_dev(ctx, graph, lst, len(lst), 3, totals(exp)), exp)
    _status(ctx, 4096)


# ---- 8: capacities ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_list_one_entry_too_long(ctx, which):
    scene = S.random_graph(12, 20, 120)
    exp = R.update_connections_list(scene.graph(), None, 3)
    caps = totals(exp)
    assert min(caps) > 3
    caps[which] -= 1
    graph = MapGraph(**scene.graph())
    got = run_dev(ctx, graph, None, len(exp), 3, caps)
    assert_equal(got, exp, truncated=True)                            # complete offsets, the first `capacity` entries, nothing past the capacity
    _status(ctx, 16384)
    with pytest.raises(OlfError) as e:                                # the host form: OLF_ERR_CAPACITY with the bit's text
        ola.UpdateConnections(graph, th=3, context=ctx, capacities=caps)
    assert e.value.code == OLF_ERR_CAPACITY and STATUS_TEXT[16384] in str(e.value)


# ---- 9: the host form ----------------------------------------------------------------------------------------------------------------------------------
def _as_lists(d):
    return {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in d.items()}


def test_host_form_equals_device_form(ctx):
    scene = S.random_graph(31, 65, 300, max_obs=40)
    graph = MapGraph(**scene.graph())
    exp = R.update_connections_list(scene.graph(), None, 15)
    assert [_as_lists(g) for g in ola.UpdateConnections(graph, context=ctx)] == exp
    check(ctx, scene, None, 15, graph=graph)
    lst = S.shuffled_list(3, 65)
    assert [_as_lists(g) for g in ola.UpdateConnections(graph, lst, th=3, context=ctx)] == R.update_connections_list(scene.graph(), lst, 3)
    (got,) = ola.UpdateConnections(MapGraph(**S.slot_rules().graph()), [1], th=1, context=ctx)
    assert _as_lists(got) == S.SLOT_RULES_EXPECTED


# ---- 10: UpdateBestCovisibles -----------------------------------------------------------------------------------------------------------------------------
def _csr(rows):
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    idx = np.asarray([k for r in rows for k in sorted(r)] + [SENTINEL] * 8, np.int32)
    w = np.asarray([r[k] for r in rows for k in sorted(r)] + [SENTINEL] * 8, np.int32)
    return off, idx, w


def _check_best(ctx, rows):
    import torch
    off, idx, w = _csr(rows)
    out = {"covis_index": torch.full((len(idx),), SENTINEL, dtype=torch.int32, device="cuda"), "covis_weight": torch.full((len(w),), SENTINEL, dtype=torch.int32, device="cuda")}
    res = connections.best_covisibles_batch(up(off), up(idx), up(w), out=out, context=ctx)
    torch.cuda.synchronize()
    want = [R.update_best_covisibles(r) for r in rows]
    assert res["covis_index"].cpu().numpy().tolist() == [k for ks, _ in want for k in ks] + [SENTINEL] * 8
    assert res["covis_weight"].cpu().numpy().tolist() == [v for _, ws in want for v in ws] + [SENTINEL] * 8
    ctx.poll_status()
    return want


def test_best_covisibles_after_reciprocal_edges(ctx):
    """the conn_* rows of a random scene with the reciprocal AddConnection calls applied on the host, in list order (:522, :529)"""
    scene = S.random_graph(41, 65, 300, max_obs=40)
    exp = R.update_connections_list(scene.graph(), None, 15)
    rows = [dict(zip(e["connected"], e["weights"])) for e in exp]
    before = [dict(r) for r in rows]
    for j, e in enumerate(exp):
        for k, w in zip(e["ordered"], e["ordered_weights"]):
            rows[k][j] = w
    assert rows != before or all(len(e["ordered"]) == e["n_counted"] for e in exp)
    want = _check_best(ctx, rows)
    assert any(len(ks) > 20 for ks, _ in want) and any(ws != sorted(set(ws), reverse=True) for _, ws in want)      # (equal weights occur)


def test_best_covisibles_rows_of_0_1_and_257(ctx):
    rng = np.random.default_rng(6)
    big = {int(k): int(rng.integers(1, 9)) for k in rng.choice(5000, 257, replace=False)}
    _check_best(ctx, [{}, {5: 3}, big, {}, {2: 1, 9: 1}])


def test_best_covisibles_row_too_long(ctx):
    import torch
    n = localmap.OLF_LOCALMAP_MAX_KF + 1
    rows = [{3: 1, 1: 2}, {k: 1 + k % 7 for k in range(n)}, {4: 4}]
    off, idx, w = _csr(rows)
    out = {"covis_index": torch.full((len(idx),), SENTINEL, dtype=torch.int32, device="cuda"), "covis_weight": torch.full((len(w),), SENTINEL, dtype=torch.int32, device="cuda")}
    res = connections.best_covisibles_batch(up(off), up(idx), up(w), out=out, context=ctx)
    torch.cuda.synchronize()
    assert res["covis_index"].cpu().numpy().tolist() == [1, 3] + [SENTINEL] * n + [4] + [SENTINEL] * 8
    assert res["covis_weight"].cpu().numpy().tolist() == [2, 1] + [SENTINEL] * n + [4] + [SENTINEL] * 8
    _status(ctx, 16384)


# ---- 11: the ordered rows go straight into the local-map call ------------------------------------------------------------------------------------------
def test_covisibility_rows_feed_update_local_map(ctx):
    import torch
    import test_localmap_gpu as tl
    scene = S.random_graph(3, 65, 300, n_frames=17, max_obs=8)
    scene.kf_covis = [[] for _ in range(65)]
    without = LR.Map(**scene.graph()).update_local_map(scene.frame_mp, scene.frame_ml)
    graph = MapGraph(**scene.graph())                                 # (kf_covis yet to be computed: empty rows)
    conn = R.update_connections_list(scene.graph(), None, 3)
    scene.kf_covis = [e["ordered"] for e in conn]
    exp = LR.Map(**scene.graph()).update_local_map(scene.frame_mp, scene.frame_ml)
    assert any(set(a["local_kfs"]) - set(b["local_kfs"]) for a, b in zip(exp, without))      # (the extension loop adds a covisible key frame)
    res = connections.update_connections_batch(graph, th=3, capacities=totals(conn), context=ctx)
    g = graph.c_dev()
    g.kf_covis_offsets, g.kf_covis_index = res["covis_offsets"].data_ptr(), res["covis_index"].data_ptr()      # device tensors, as they are
    fmp, cnt = tl.rows(ctx, scene.frame_mp, ctx.orb_capacity, 1, 0)
    caps = [sum(len(e[k]) for e in exp) for k in ("local_kfs", "local_points", "local_lines")]
    out = localmap.update_local_map_batch(g, len(exp), up(fmp), up(cnt), capacities=caps, context=ctx)
    torch.cuda.synchronize()
    got = {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}
    for k, key in (("kf", "local_kfs"), ("mp", "local_points")):
        assert np.array_equal(got[k + "_offsets"], np.concatenate([[0], np.cumsum([len(e[key]) for e in exp])])), k
        assert got[k + "_index"][:got[k + "_offsets"][-1]].tolist() == [v for e in exp for v in e[key]], k
    assert [int(v) for v in got["ref_kf"]] == [e["ref_kf"] for e in exp]
    ctx.poll_status()


# ---- 12: the reference-side adaptor on the device ------------------------------------------------------------------------------------------------------
def test_adaptor_update_connections(tmp_path):
    from test_connections_cpu import build_adaptor
    exe = str(tmp_path / "adaptor_connections")
    build_adaptor(exe)
    out = subprocess.run([exe, "device"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"ADAPTOR_CONNECTIONS_OK" in out.stdout, out.stdout.decode()[-3000:]
