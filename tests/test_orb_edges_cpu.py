"""Every scene of tests/orb_edge_scenes.py reaches, on the CPU oracle, the path it is named for: a scene that no longer does fails here and cannot pass
silently on the device (tests/test_orb_edges_gpu.py runs the same scenes against the library)."""
import numpy as np
import pytest
import orb_edge_scenes as S

_run = S.oracle_run


def _cells(o, level):
    return S.cell_stats(o["candidates"][level], *o["sizes"][level])


def _classes(o):
    z = o["sizes"]
    return [S.resize_class(*z[l - 1], *z[l]) for l in range(1, len(z))]


@pytest.mark.parametrize("name", list(S.SCENES))
def test_scene_runs_in_under_a_second(oracle, name):
    s = S.SCENES[name]
    o = _run(oracle, name)
    assert np.array_equal(s.image(), s.image())      # a fixed seed
    assert o["seconds"] < 1.0
    assert len(o["sizes"]) == s.nlevels and min(min(z) for z in o["sizes"]) >= 62


def test_min_level(oracle):
    o = _run(oracle, "min_level")
    assert o["sizes"][3] == (74, 62) and S.cell_grid(74, 62)[:2] == (1, 1)
    assert len(o["candidates"][3]) > 0


def test_one_cell_64(oracle):
    o = _run(oracle, "one_cell_64")
    assert S.cell_grid(64, 64) == (1, 1, 32, 32)
    assert len(o["kps"]) == 50


def test_odd(oracle):
    o = _run(oracle, "odd")
    assert o["sizes"] == [(131, 97), (109, 81), (91, 67)]
    assert 59 in [S.cell_grid(*z)[2] for z in o["sizes"]]
    # more than 64 survivors in a cell is k_cells_sort's LDS path, more than 128 its second sort size; the device counts a cell before the dual threshold
    # drops anything, so it holds at least what the oracle kept.  (More than 256 per cell is not reached: noise gave at most 190 in these scenes.)
    assert max(_cells(o, l)[0].max() for l in range(3)) > 128


def test_odd_203(oracle):
    o = _run(oracle, "odd_203")
    # widths 203, 169, 141, 117 and 98: four odd ones of both residues mod 4 and one that is even, none a multiple of 4
    assert [w for w, _ in o["sizes"]] == [203, 169, 141, 117, 98]
    assert {w % 4 for w, _ in o["sizes"]} == {1, 2, 3}
    assert all(len(c) > 0 for c in o["candidates"])


def test_resize_classes(oracle):
    assert _classes(_run(oracle, "sf2")) == ["generic", "strip"]
    # the LDS-tiled kernel: the strip kernel covers every factor up to 2 and the tile's 16 staged rows none much beyond it, so it is left with levels whose
    # width is 2 n + 1 -> n (a factor just above 2) and at most 190 columns (its 96 staged words)
    o = _run(oracle, "sf2_tiled")
    assert _classes(o) == ["tiled"] and o["sizes"] == [(301, 200), (150, 100)]
    o = _run(oracle, "sf2_tiled_full")
    assert _classes(o) == ["tiled"] and o["sizes"] == [(381, 200), (190, 100)]
    assert min(S._axis_ofs(381, 190, True)[-1] + 1, 380) // 4 + 1 == 96
    assert all(len(c) > 0 for c in o["candidates"])
    assert _classes(_run(oracle, "sf3")) == ["generic"]
    o = _run(oracle, "sf19")
    assert _classes(o) == ["generic"] and o["sizes"][1] == (211, 105)
    assert _classes(_run(oracle, "sf15")) == ["strip", "strip"]
    o = _run(oracle, "sf11")
    assert len(o["sizes"]) == 12 and _classes(o) == ["strip"] * 11
    assert all(len(c) > 0 for c in o["candidates"])
    # the default scale factor takes the strip kernel on every level as well: the other two kernels are reached by these scenes alone
    assert set(_classes(_run(oracle, "odd_203"))) == {"strip"}


@pytest.mark.parametrize("name,w,h,roots", [("ratio15", 122, 92, 2), ("ratio25", 182, 92, 3)])
def test_root_count_at_exact_halves(oracle, name, w, h, roots):
    o = _run(oracle, name)
    assert o["sizes"] == [(w, h)]
    assert (w - 32) / (h - 32) == roots - 0.5 and S.n_ini(w, h) == roots
    assert len(o["kps"]) > 0


def test_both_branches(oracle):
    o = _run(oracle, "both_branches")
    ok = False
    for l in range(4):
        count, best = _cells(o, l)
        ok |= bool((best >= 20).any() and ((count > 0) & (best < 20)).any())
    assert ok


def test_binary_thresholds(oracle):
    a, b, c = _run(oracle, "binary_254"), _run(oracle, "binary_254_254"), _run(oracle, "binary_1")
    for o in (a, b, c):
        assert len(o["candidates"][0]) > 0 and (o["candidates"][0][:, 2] == 254).all()
    assert _cells(a, 0)[1].max() < 255 and len(a["kps"]) > 0                      # no cell reaches ini = 255
    assert np.array_equal(a["candidates"][0], b["candidates"][0])                 # the same corners through the ini branch
    assert np.array_equal(a["kps"], b["kps"]) and np.array_equal(a["desc"], b["desc"])
    assert np.array_equal(a["candidates"][0], c["candidates"][0])
    assert len(c["candidates"][1]) > 0 and c["candidates"][1][:, 2].min() == 1    # threshold 1 keeps scores of 1 on the resized level


def test_none(oracle):
    o = _run(oracle, "none")
    assert len(o["kps"]) == 0 and o["desc"].shape == (0, 32) and all(len(c) == 0 for c in o["candidates"])


def test_ini_below_min(oracle):
    """the retry at min finds nothing where FAST at ini found nothing, so (7, 20) keeps what (7, 7) keeps"""
    o, lo, hi = _run(oracle, "ini_below_min"), _run(oracle, "ini_below_min", 7, 7), _run(oracle, "ini_below_min", 20, 20)
    for l in range(2):
        assert len(o["candidates"][l]) > 0 and np.array_equal(o["candidates"][l], lo["candidates"][l])
        assert len(hi["candidates"][l]) < len(o["candidates"][l])
        assert o["candidates"][l][:, 2].min() == 7
    assert np.array_equal(o["kps"], lo["kps"]) and np.array_equal(o["desc"], lo["desc"])


def test_small_quotas(oracle):
    o = _run(oracle, "small_quota")
    assert len(o["kps"]) > 20
    o = _run(oracle, "quota_one")
    per_level = np.bincount(o["kps"]["octave"], minlength=2)
    assert per_level[0] > 1 and per_level[1] > 1


def test_widest(oracle):
    o = _run(oracle, "widest")
    assert o["sizes"] == [(S.MAX_SIDE, 96)]
    assert o["candidates"][0][:, 0].max() == 4095 == S.MAX_SIDE - 36


def test_one_pixel_wider_does_not_fit(oracle):
    """the largest candidate coordinate is the side - 36 (the same arithmetic along y): 4096 at 4132 pixels, one more than 12 bits hold"""
    p = oracle.orb_params(3000, 1.2, 1, 20, 7)
    o = oracle.orb_extract(S.noise(119, S.MAX_SIDE + 1, 96), p, debug=True, cap=8192)
    assert o["candidates"][0][:, 0].max() == 4096
