#!/usr/bin/env python3
"""Regenerates tests/golden/reference_containers.npz, tests/golden/stereo_line_edges.npz and tests/golden/reference_config.json: what the
reference's own STL-only code returns on the inputs of tests/test_oracle_cpu.py and on the border, cell-boundary, steep and clipped lines of
tests/stereo_line_scenes.py (tests/test_stereo_lines_cpu.py), and the defaults of its Config / KITTI settings file
that tests/test_host_cpu.py checks olf_default_params against.  The tests compare against these recorded results, so
they do not need the reference checkout; where oracle/_ref is built they also check the live reference against them.

    python tests/golden/make_reference_golden.py <reference checkout>

oracle/_ref/libref_grid.so and libref_bow.so must have been built first (make -C oracle ref REF=<reference checkout>)."""
import ctypes as C
import json
import os
import re
import sys
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as oracle
import stereo_line_scenes

GOLDEN = os.path.join(ROOT, "tests", "golden")


def line_iterator_cases():
    rng = np.random.default_rng(3)
    cases = [(0.0, 0.0, 63.9, 47.9), (10.5, 3.2, 10.5, 40.0), (5.0, 5.0, 5.0, 5.0), (60.2, 1.0, 2.0, 1.9), (3.3, 44.0, 3.9, 2.0)]
    cases += [tuple(rng.uniform(-2, 66, 4)) for _ in range(400)]
    return np.array(cases, np.float64)


def grid_query_trials():
    rng = np.random.default_rng(4)
    out = []
    for _ in range(60):
        n = int(rng.integers(1, 120))
        segs = np.ascontiguousarray(rng.uniform(-1, 65, (n, 4)) * np.array([1, 0.75, 1, 0.75]))
        q = rng.integers(-2, 66, 4)
        out.append((segs, q))
    return out


def stereo_line_edges(grid):
    """getLineCoords' cell lists and GridStructure::get's candidates (iteration order included) on stereo_line_scenes.edge_inputs()"""
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    cases, trials = stereo_line_scenes.edge_inputs()
    buf, xy, offs = np.zeros((4096, 2), np.int32), [], [0]
    for x1, y1, x2, y2 in cases:
        n = grid.ref_line_coords(C.c_double(x1), C.c_double(y1), C.c_double(x2), C.c_double(y2), P(buf), 4096)
        xy.append(buf[:n].copy()); offs.append(offs[-1] + n)
    rec = dict(line_cases=cases, line_xy=np.concatenate(xy), line_offs=np.array(offs, np.int64))
    a = np.zeros(4096, np.int32)
    for t, (segs, queries) in enumerate(trials):
        cand, coffs = [], [0]
        for spx, spy, epx, epy, ws in queries:
            na = grid.ref_grid_query(48, 64, P(segs), len(segs), int(spx), int(spy), int(ws), 0, 0, 0, int(epx), int(epy), 1, P(a), 4096)
            cand.append(a[:na].copy()); coffs.append(coffs[-1] + na)
        rec.update({f"grid{t}_segs": segs, f"grid{t}_q": queries, f"grid{t}_cand": np.concatenate(cand), f"grid{t}_cand_offs": np.array(coffs, np.int64)})
    rec["n_trials"] = np.int64(len(trials))
    np.savez_compressed(os.path.join(GOLDEN, "stereo_line_edges.npz"), **rec)
    return len(cases), sum(len(q) for _, q in trials)


def bow_inputs():
    """(feats, [(scoring, weighting, word, w, node)]) exactly as test_bow_oracle_vs_reference_containers draws them"""
    rng = np.random.default_rng(12)
    k, L = 4, 3
    parent, leaf, desc, weight = oracle.random_vocabulary(k, L, 5, tie_every=7, stop_every=9)
    feats = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    feats[:40] = desc[np.flatnonzero(leaf)[rng.integers(0, leaf.sum(), 40)]]
    combos = []
    for scoring in range(6):
        for weighting in range(4):
            V = oracle.OracleVoc.create(k, L, parent, leaf, desc, weight, scoring, weighting)
            word, w, node = V.words(feats, 1)
            combos.append((scoring, weighting, np.ascontiguousarray(word, np.int32), np.ascontiguousarray(w, np.float64), np.ascontiguousarray(node, np.int32)))
    return feats, combos


def ref_bow_args(scoring, weighting):
    """ref_bow_build's mode / divide_by_size / norm for one scoring x weighting (TemplatedVocabulary::transform's branches)"""
    must, tf = scoring != 5, weighting in (0, 1)
    return 0 if tf else 1, int(tf and not must), (1 if scoring == 1 else 0) if must else -1


# the Config defaults and KITTI settings tests/test_host_cpu.py compares olf_default_params with
CONFIG_KEYS = ("min_disp", "line_sim_th", "stereo_overlap_th", "line_horiz_th", "min_ratio_12_l", "ls_min_disp_ratio", "best_lr_matches", "matching_s_ws",
               "min_line_length", "lsd_refine", "lsd_scale", "lsd_sigma_scale", "lsd_quant", "lsd_ang_th", "lsd_log_eps", "lsd_density_th", "lsd_n_bins")
KITTI_KEYS = ("ORBextractor.nFeatures", "ORBextractor.scaleFactor", "ORBextractor.nLevels", "ORBextractor.iniThFAST", "ORBextractor.minThFAST",
              "Camera.fx", "Camera.bf", "lsd_nfeatures")


def main(ref_checkout):
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    grid = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_grid.so"))
    bowl = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref_bow.so"))
    rec = {}
    # LineIterator.cpp getLineCoords: the (x, y) list of every case, concatenated
    cases = line_iterator_cases()
    buf, xy, offs = np.zeros((4096, 2), np.int32), [], [0]
    for x1, y1, x2, y2 in cases:
        n = grid.ref_line_coords(C.c_double(x1), C.c_double(y1), C.c_double(x2), C.c_double(y2), P(buf), 4096)
        xy.append(buf[:n].copy()); offs.append(offs[-1] + n)
    rec.update(line_cases=cases, line_xy=np.concatenate(xy), line_offs=np.array(offs, np.int64))
    # gridStructure.cpp: the candidate set of every query in std::unordered_set iteration order
    segs_all, segs_offs, qs, cand, cand_offs = [], [0], [], [], [0]
    a = np.zeros(4096, np.int32)
    for segs, q in grid_query_trials():
        n = len(segs)
        na = grid.ref_grid_query(48, 64, P(segs), n, int(q[0]), int(q[1]), 10, 0, 0, 0, int(q[2]), int(q[3]), 1, P(a), 4096)
        segs_all.append(segs); segs_offs.append(segs_offs[-1] + n); qs.append(q)
        cand.append(a[:na].copy()); cand_offs.append(cand_offs[-1] + na)
    rec.update(grid_segs=np.concatenate(segs_all), grid_segs_offs=np.array(segs_offs, np.int64), grid_q=np.array(qs, np.int64),
               grid_cand=np.concatenate(cand), grid_cand_offs=np.array(cand_offs, np.int64))
    # DBoW2 BowVector / FeatureVector: the containers built from the oracle's words, for every scoring x weighting
    _, combos = bow_inputs()
    fields = {k: [] for k in ("bow_word", "bow_w", "bow_node", "bow_ids", "bow_vals", "fv_nodes", "fv_offs", "fv_idx")}
    counts = []
    for scoring, weighting, word, w, node in combos:
        ids, vals = np.zeros(300, np.int32), np.zeros(300, np.float64)
        nb = bowl.ref_bow_build(P(word), P(w), 300, *ref_bow_args(scoring, weighting), P(ids), P(vals))
        nodes, foffs, idx = np.zeros(300, np.int32), np.zeros(301, np.int32), np.zeros(300, np.int32)
        nf = bowl.ref_fv_build(P(node), P(w), 300, P(nodes), P(foffs), P(idx))
        for k, v in (("bow_word", word), ("bow_w", w), ("bow_node", node), ("bow_ids", ids[:nb]), ("bow_vals", vals[:nb]), ("fv_nodes", nodes[:nf]),
                     ("fv_offs", foffs[:nf + 1]), ("fv_idx", idx[:foffs[nf]])):
            fields[k].append(v)
        counts.append((scoring, weighting, nb, nf, foffs[nf]))
    rec.update({k: np.concatenate(v) for k, v in fields.items()})
    rec["bow_counts"] = np.array(counts, np.int64)
    np.savez_compressed(os.path.join(GOLDEN, "reference_containers.npz"), **rec)
    n_edge_lines, n_edge_queries = stereo_line_edges(grid)

    # Config::Config() defaults (src/Config.cpp) and the KITTI settings file of the PL example, as name -> value
    text = open(os.path.join(ref_checkout, "src", "Config.cpp"), encoding="utf-8", errors="replace").read()
    cfg = {}
    for name, val in re.findall(r"^\s*(\w+)\s*=\s*([-+0-9.eE]+|true|false)\s*;", text, re.M):
        cfg.setdefault(name, {"true": 1.0, "false": 0.0}[val] if val in ("true", "false") else float(val))
    yml = open(os.path.join(ref_checkout, "Examples", "PL", "PL_KITTI00-02.yaml"), errors="replace").read()
    kitti = dict(re.findall(r"^([\w.]+)\s*:\s*([-+0-9.eE]+)\s*(?:#.*)?$", yml, re.M))
    with open(os.path.join(GOLDEN, "reference_config.json"), "w") as f:
        json.dump({"Config.cpp": {k: cfg[k] for k in CONFIG_KEYS}, "PL_KITTI00-02.yaml": {k: kitti[k] for k in KITTI_KEYS}}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(n_edge_lines, "edge line cases,", n_edge_queries, "edge grid queries,")
    print(len(cases), "line cases,", len(qs), "grid queries,", len(combos), "BoW combinations,", len(CONFIG_KEYS), "Config defaults,", len(KITTI_KEYS), "KITTI settings")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
