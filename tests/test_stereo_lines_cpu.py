"""CPU tests (no GPU) of the constructed stereo-line scenes (tests/stereo_line_scenes.py): that they take the oracle where
tests/test_stereo_lines_gpu.py needs it to go -- matches, accepted disparities, an answer that moves with every Config key, an infinite disparity,
no NaN -- that each hand-written scene has its stated answer, and that the oracle's grid (line_coords, orc_grid_query) agrees with what the
reference's own getLineCoords / GridStructure return on the scenes' border, cell-boundary, steep and clipped lines
(tests/golden/stereo_line_edges.npz, recorded by tests/golden/make_reference_golden.py; oracle/_ref, where built, is checked against the record)."""
import ctypes as C
import os
import numpy as np
import pytest
import stereo_line_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = S.HAND_W, S.HAND_H


def _run(oracle, sc, ps=None, w=W, h=H):
    p = S.apply_params(oracle.full_params(50, S.CAP), ps or {})
    return oracle.stereo_lines(*sc, w, h, p.stereo)


def _differs(a, b):
    return (not np.array_equal(a[0], b[0]) or not np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) or
            not np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)))


def test_scene_builder_is_seeded_and_bounded():
    a, b = S.scene(S.SEED, 65, 129, W, H), S.scene(S.SEED, 65, 129, W, H)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert [len(x) for x in a] == [65, 65, 129, 129] and a[1].dtype == np.uint8 and a[1].shape == (65, 32)
    kinds = S.scene_kinds(S.SEED, S.CAP)
    assert set(kinds) == set(S.KINDS)                                   # the (160, 160) scene draws every kind
    klL = S.cached_scene(S.SEED, S.CAP, S.CAP, W, H)[0]
    seg = S.segs_of(klL)
    assert (seg[:, [0, 2]] == W).any() and (seg[:, [1, 3]] == H).any()   # clipped end points at x == W and y == H
    cells = np.trunc(S.grid_segs(klL, W, H)).astype(int)
    assert ((cells[:, 0] == cells[:, 2]) & (cells[:, 1] == cells[:, 3])).any()      # a left line inside one cell: the 0 / 0 direction
    klR = S.cached_scene(S.SEED, S.CAP, S.CAP, W, H)[2]
    assert (klR["startPointY"] == klR["endPointY"]).any()               # an exactly horizontal right line: the division by zero
    assert S.dist_wave_max_pairs() == 256


def test_default_parameters_match_and_accept(oracle):
    m, disp, le = _run(oracle, S.cached_scene(S.SEED, S.CAP, S.CAP, W, H))
    assert (m >= 0).sum() >= 60 and (disp[:, 0] >= 0).sum() >= 10
    for sh in S.SHAPES:
        m, disp, le = _run(oracle, S.cached_scene(S.SEED, *sh, W, H))
        assert len(m) == sh[0] and not np.isnan(disp).any() and not np.isnan(le).any()
        if 0 in sh:
            assert (m == -1).all()


@pytest.mark.parametrize("ps", S.PARAM_SETS, ids=S.param_id)
def test_every_parameter_set_changes_the_answer(oracle, ps):
    changed = False
    for sh in S.SWEEP_SHAPES:
        sc = S.cached_scene(S.SEED, *sh, W, H)
        out = _run(oracle, sc, ps)
        assert not np.isnan(out[1]).any() and not np.isnan(out[2]).any()          # a NaN's sign and payload are no defined target
        changed = changed or _differs(out, _run(oracle, sc))
    assert changed


def test_an_infinite_disparity_reaches_the_output(oracle):
    """an exactly horizontal right line divides by zero; with a negative stereo_overlap_th the pair is accepted with both disparities +inf"""
    inf = 0
    for sh in S.SWEEP_SHAPES:
        m, disp, le = _run(oracle, S.cached_scene(S.SEED, *sh, W, H), dict(stereo_overlap_th=-1.0))
        rows = np.isinf(disp).any(1)
        assert (disp[rows] == np.inf).all() and np.isfinite(le[rows]).all()
        inf += int(rows.sum())
    assert inf >= 1


@pytest.mark.parametrize("size", [(S.HAND_W, S.HAND_H), (333, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", sorted(S.hand_scenes()))
def test_hand_written_scenes(oracle, name, size):
    h = S.hand_scenes(*size)[name]
    m, disp, le = _run(oracle, (h["klL"], h["descL"], h["klR"], h["descR"]), w=size[0], h=size[1])
    assert np.array_equal(m, h["m12"])
    if h["disp"] is not None:
        assert np.array_equal(disp, h["disp"])
    assert ((disp[:, 0] >= 0) <= (m >= 0)).all()


@pytest.mark.parametrize("variant", ["a", "b"])
@pytest.mark.parametrize("nL", S.STAIR_NL)
def test_staircase_winner(oracle, nL, variant):
    """every left line reaches the one right line; the first line with the smallest distance holds it in the end"""
    d = S.staircase_distances(nL, variant)
    rec = np.flatnonzero(d < np.minimum.accumulate(np.concatenate([[1 << 30], d[:-1]])))       # the strict records, in order
    assert rec[0] == 0 and (nL < 64 or 63 in rec)                      # lane 0 and lane 63 of the first wave step
    if nL > 64:
        assert (64 in rec) == (variant == "a") and (d[64] == d[63]) == (variant == "b")
    m, disp, le = _run(oracle, S.staircase(nL, variant, 333, 257), S.STAIR_PARAMS, 333, 257)
    want = np.full(nL, -1, np.int32)
    want[S.staircase_winner(nL, variant)] = 0
    assert rec[-1] == S.staircase_winner(nL, variant) and np.array_equal(m, want)
    # without the left-right check every line takes the right line (one candidate: nothing to lose the ratio test to)
    m0, _, _ = _run(oracle, S.staircase(nL, variant, 333, 257), dict(S.STAIR_PARAMS, best_lr_matches=0), 333, 257)
    assert (m0 == 0).all()


@pytest.mark.parametrize("size", [(333, 257), (1000, 300), (401, 243), (897, 601)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_border_scene_matches(oracle, size):
    w, h = size
    sc = S.border_scene(w, h)
    seg = S.segs_of(sc[0])
    assert (seg[:, [0, 2]] == w).any() and (seg[:, [1, 3]] == h).any() and (seg == 0).any()
    p = oracle.full_params(700, 150, 400.0, 40.0)
    m, disp, le = oracle.stereo_lines(*sc, w, h, p.stereo)
    assert (m >= 0).sum() >= 8 and (disp[:, 0] >= 0).sum() >= 3 and not np.isnan(disp).any() and not np.isnan(le).any()


# ---- the oracle's grid against the reference's own code on these inputs --------------------------------------------------------------------------
def _ref_grid():
    p = os.path.join(ROOT, "oracle", "_ref", "libref_grid.so")
    return C.CDLL(p) if os.path.exists(p) else None


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "stereo_line_edges.npz"))


def test_edge_line_coords_match_reference(oracle):
    ref, g = _ref_grid(), _golden()
    cases, trials = S.edge_inputs()
    assert np.array_equal(g["line_cases"], cases) and len(cases) > 100           # the record is of these scenes
    xy, offs = g["line_xy"], g["line_offs"]
    buf = np.zeros((4096, 2), np.int32)
    kinds = dict(cell_64=0, row_48=0, steep=0, outside=0)
    for i, (x1, y1, x2, y2) in enumerate(cases):
        want = xy[offs[i]:offs[i + 1]]
        assert np.array_equal(oracle.line_coords(x1, y1, x2, y2), want), i
        if ref is not None:
            n = ref.ref_line_coords(C.c_double(x1), C.c_double(y1), C.c_double(x2), C.c_double(y2), buf.ctypes.data_as(C.c_void_p), 4096)
            assert np.array_equal(buf[:n], want), i
        kinds["cell_64"] += int((want[:, 0] == 64).any()); kinds["row_48"] += int((want[:, 1] == 48).any())
        kinds["steep"] += int(abs(y2 - y1) > abs(x2 - x1)); kinds["outside"] += int((want < 0).any() or (want[:, 0] > 64).any())
    assert kinds["cell_64"] >= 3 and kinds["row_48"] >= 3 and kinds["steep"] >= 20, kinds


def test_edge_grid_queries_match_reference(oracle):
    ref, g = _ref_grid(), _golden()
    cases, trials = S.edge_inputs()
    assert int(g["n_trials"]) == len(trials)
    a, b = np.zeros(4096, np.int32), np.zeros(4096, np.int32)
    nonempty = 0
    for t, (segs, queries) in enumerate(trials):
        assert np.array_equal(g[f"grid{t}_segs"], segs) and np.array_equal(g[f"grid{t}_q"], queries)
        assert set(queries[:, 4]) == set(S.EDGE_WS)
        cand, co = g[f"grid{t}_cand"], g[f"grid{t}_cand_offs"]
        segs = np.ascontiguousarray(segs)
        for k, (spx, spy, epx, epy, ws) in enumerate(queries):
            want = cand[co[k]:co[k + 1]]
            args = (48, 64, segs.ctypes.data_as(C.c_void_p), len(segs), int(spx), int(spy), int(ws), 0, 0, 0, int(epx), int(epy), 1)
            nb = oracle._L.orc_grid_query(*args, b.ctypes.data_as(C.c_void_p), 4096)
            assert np.array_equal(b[:nb], want), (t, k)                  # same set and same unordered_set iteration order
            if ref is not None:
                na = ref.ref_grid_query(*args, a.ctypes.data_as(C.c_void_p), 4096)
                assert np.array_equal(a[:na], want), (t, k)
            nonempty += int(len(want) > 0)
    assert nonempty >= 100
