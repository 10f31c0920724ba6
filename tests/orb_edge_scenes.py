"""Named scenes for the ORB extractor at small, odd, wide and off-default settings (tests/test_orb_edges_cpu.py asserts on the oracle that each scene
reaches the path it is named for; tests/test_orb_edges_gpu.py compares the device with the oracle on the same scenes, stage by stage).

A scene is an image builder with a fixed seed, the constructor arguments (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST) and the property it must
reach.  The geometry helpers restate the host tables of the extractor (the FAST cell grid, the root count of DistributeOctTree, and which of the three resize
kernels a pyramid level takes) in plain numpy, so that a scene can say which device path it pins without asking the library."""
import functools
import time
from collections import namedtuple
import numpy as np

MIN_BORDER = 16          # EDGE_THRESHOLD - 3: candidates are reported relative to this border
MAX_SIDE = 4131          # widest / highest level 0 whose candidate coordinates (at most side - 36) fit the 12-bit fields of the packed candidate word

Scene = namedtuple("Scene", "name image nfeatures scale nlevels ini min")


def noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def low_contrast(seed, w, h):
    """noise // 6 + 100: FAST scores of at most 41, most of them below 20 -- both branches of the dual threshold on one level"""
    return (noise(seed, w, h) // 6 + 100).astype(np.uint8)


def binary(seed, w, h):
    """pixels 0 or 255 only: every corner scores exactly 254, the extreme of the SWAR pre-test's fields"""
    return (np.random.default_rng(seed).integers(0, 2, (h, w), dtype=np.uint8) * 255).astype(np.uint8)


_S = lambda name, build, seed, w, h, *p: Scene(name, functools.partial(build, seed, w, h), *p)

SCENES = {s.name: s for s in [
    #  name              image                       nfeatures scale nlevels ini  min
    _S("min_level",      noise, 101, 128, 107,       100, 1.2, 4, 20, 7),       # top level 74 x 62: the smallest accepted, a 1 x 1 cell grid
    _S("one_cell_64",    noise, 102, 64, 64,         50, 1.2, 1, 20, 7),        # 1 x 1 grid of a 32 x 32 cell, the quota is reached
    _S("odd",            noise, 103, 131, 97,        200, 1.2, 3, 20, 7),       # levels 109 x 81 and 91 x 67; a 59-pixel cell; a cell with > 128 survivors
    _S("odd_203",        noise, 104, 203, 151,       300, 1.2, 5, 20, 7),       # five levels, widths 203, 169, 141, 117, 98: none a multiple of 4
    _S("sf2",            noise, 105, 517, 259,       500, 2.0, 3, 20, 7),       # level 1 generic resize, level 2 strip
    _S("sf2_tiled",      noise, 121, 301, 200,       300, 2.0, 2, 20, 7),       # 301 -> 150 columns is a factor of 2.007: strip does not fit, the LDS-tiled kernel does
    _S("sf2_tiled_full", noise, 122, 381, 200,       300, 2.0, 2, 20, 7),       # the same with 190 columns: the tile's 96 staged words are all used
    _S("sf3",            noise, 106, 640, 300,       500, 3.0, 2, 20, 7),       # generic resize
    _S("sf19",           noise, 107, 400, 200,       500, 1.9, 2, 20, 7),       # generic resize, level 1 is 211 x 105
    _S("sf15",           noise, 108, 333, 201,       500, 1.5, 3, 20, 7),       # strip at the largest scale at which strip is confirmed
    _S("sf11",           noise, 109, 401, 263,       600, 1.1, 12, 20, 7),      # twelve levels
    _S("ratio15",        noise, 110, 122, 92,        100, 1.2, 1, 20, 7),       # (W - 32) / (H - 32) = 1.5 exactly: nIni rounds to 2
    _S("ratio25",        noise, 111, 182, 92,        100, 1.2, 1, 20, 7),       # 2.5 exactly: nIni = 3
    _S("both_branches",  low_contrast, 112, 203, 151, 300, 1.2, 4, 20, 7),      # cells with a score >= ini beside non-empty cells without one
    _S("binary_254",     binary, 113, 131, 97,       200, 1.2, 2, 255, 254),    # every level-0 score is 254: the min retry everywhere
    _S("binary_254_254", binary, 113, 131, 97,       200, 1.2, 2, 254, 254),    # the same corners through the ini branch
    _S("binary_1",       binary, 113, 131, 97,       200, 1.2, 2, 255, 1),      # threshold 1, the other end of the SWAR bound
    _S("none",           noise, 114, 160, 120,       300, 1.2, 2, 255, 200),    # zero key points, no error
    _S("ini_below_min",  low_contrast, 115, 160, 120, 300, 1.2, 2, 7, 20),      # the reference keeps every corner with score >= ini
    _S("small_quota",    noise, 116, 640, 100,       20, 1.2, 1, 20, 7),        # more key points than nfeatures (first octree sweep splits all roots)
    _S("quota_one",      noise, 117, 640, 100,       1, 1.2, 2, 20, 7),         # the same on two levels
    _S("widest",         noise, 118, MAX_SIDE, 96,   3000, 1.2, 1, 20, 7),      # a candidate at x = 4095, the last value that fits
]}


# ---- geometry of a level, as the extractor's host tables compute it ---------------------------------------------------------------------------------

def cell_grid(w, h):
    """(nCols, nRows, wCell, hCell) of ComputeKeyPointsOctTree for a w x h level (float32 arithmetic, as the reference)"""
    width, height = np.float32(w - 2 * MIN_BORDER), np.float32(h - 2 * MIN_BORDER)
    n_cols, n_rows = int(width / np.float32(30)), int(height / np.float32(30))
    return n_cols, n_rows, int(np.ceil(width / np.float32(n_cols))), int(np.ceil(height / np.float32(n_rows)))


def n_ini(w, h):
    """root nodes of DistributeOctTree: std::round (half away from zero) of the float ratio of the bordered level"""
    return int(np.floor(float(np.float32(w - 2 * MIN_BORDER) / np.float32(h - 2 * MIN_BORDER)) + 0.5))


def cell_stats(cand, w, h):
    """per-cell candidate count and maximum score, (nRows, nCols) each, of one level's oracle candidates (x, y, score); x and y are relative to the border
    and a cell's interior starts 3 pixels inside its sub-image"""
    n_cols, n_rows, w_cell, h_cell = cell_grid(w, h)
    count, best = np.zeros((n_rows, n_cols), np.int64), np.zeros((n_rows, n_cols), np.int64)
    cj, ci = (cand[:, 0] - 3) // w_cell, (cand[:, 1] - 3) // h_cell
    assert len(cand) == 0 or (cj.min() >= 0 and cj.max() < n_cols and ci.min() >= 0 and ci.max() < n_rows)
    np.add.at(count, (ci, cj), 1)
    np.maximum.at(best, (ci, cj), cand[:, 2])
    return count, best


def _axis_ofs(sn, dn, clamp):
    """first source tap of every output position of cv::resize(INTER_LINEAR) with an explicit dsize (scale = 1 / (dn / sn) in double, position in float)"""
    scale = 1.0 / (dn / sn)
    s = np.floor(((np.arange(dn, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)).astype(np.int64)
    return np.clip(s, 0, sn - 1) if clamp else s


def resize_class(sw, sh, dw, dh):
    """which kernel resizes an sw x sh level to dw x dh: 'strip' (registers only: every quad of output columns finds its source bytes inside 8 consecutive
    bytes), 'tiled' (a 256 x 8 output tile's source window fits 96 words x 16 rows of LDS) or 'generic'"""
    rx, ry = _axis_ofs(sw, dw, True), _axis_ofs(sh, dh, False)
    for x0 in range(0, dw, 256):
        nx = min(256, dw - x0)
        if (min(rx[x0 + nx - 1] + 1, sw - 1) - (rx[x0] & ~3)) // 4 + 1 > 96:
            return "generic"
    for y0 in range(0, dh, 8):
        ny = min(8, dh - y0)
        r0, r1 = min(max(ry[y0], 0), sh - 1), min(max(ry[y0 + ny - 1] + 1, 0), sh - 1)
        if r1 - r0 + 1 > 16:
            return "generic"
    if sw < 8:
        return "tiled"
    for x0 in range(0, dw, 4):
        if min(rx[min(x0 + 3, dw - 1)] + 1, sw - 1) - rx[x0] > 7:
            return "tiled"
    return "strip"


# ---- the reference of both test files -------------------------------------------------------------------------------------------------------------

_RUNS = {}


def oracle_run(oracle, name, ini=None, mn=None):
    """the oracle's debug run of a scene (optionally at other thresholds), computed once per session and shared: callers must not modify it.  Besides
    orb_extract's outputs it holds the image, the level sizes and the wall time of the run."""
    key = (name, ini, mn)
    if key not in _RUNS:
        s = SCENES[name]
        img = s.image()
        p = oracle.orb_params(s.nfeatures, s.scale, s.nlevels, s.ini if ini is None else ini, s.min if mn is None else mn)
        t = time.perf_counter()
        o = oracle.orb_extract(img, p, debug=True, cap=s.nfeatures + 4096)
        o["seconds"] = time.perf_counter() - t
        lw, lh = oracle.orb_level_sizes(p, img.shape[1], img.shape[0])
        o["sizes"] = list(zip(lw.tolist(), lh.tolist()))
        o["image"] = img
        _RUNS[key] = o
    return _RUNS[key]
