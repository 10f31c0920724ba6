"""Latency of place recognition for a batch of queries: olf_kfdb_tables_dev (csrc/kfdb.hip; queries and tables stay on the device) and olf_kfdb_detect (host
pointers in, candidate lists out: upload, tables, download, selection), both relocalisation forms, beside a plain C++ restatement of the reference's own
walk (tools/kfdb_host_walk.cpp: a std::list inverted file, std::map vectors; compiled -O3 here, one host thread) that stands for the reference, which the
repository cannot compile.  Databases of 500 and 4000 key frames of about 1500 point words out of 10^6 ids and 400 line words out of 10^5; each key frame's
ten predecessors are its best covisibles; a query is a key frame's vector with half of its words replaced.  Q = 1, 8 and 64 queries per call.
python tools/kfdb_latency.py [--kfs 500,4000] [--queries 1,8,64]
olf_kfdb_tables_dev: HIP events, warmed up, median of five windows of ten calls.  olf_kfdb_detect and the host walk return to the host, so they are timed by
the host clock over the same windows (detect ends in a synchronise).  The candidate lists of the two are compared."""
import argparse, ctypes as C, os, subprocess, tempfile, time
import numpy as np
from latency_common import ROOT, side_stream, windows
import torch
from orb_line_slam_amd import _lib
from orb_line_slam_amd._lib import BowCsrC, KfdbTablesC, KFDB_RELOC, KFDB_RELOC_LINE, check, lib
from orb_line_slam_amd.database import KeyFrameDatabase, _lists_csr, bow_csr

ap = argparse.ArgumentParser()
ap.add_argument("--kfs", default="500,4000")
ap.add_argument("--queries", default="1,8,64")
ap.add_argument("--words", type=int, default=1500)
ap.add_argument("--line-words", type=int, default=400)
args = ap.parse_args()
NP, NL = 10**6, 10**5

tmp = tempfile.mkdtemp()
so = os.path.join(tmp, "libkfdb_host_walk.so")
subprocess.run(["g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "kfdb_host_walk.cpp")], check=True)
HW = C.CDLL(so)
HW.hw_create.restype = C.c_void_p
HW.hw_create.argtypes = [C.c_int, C.c_int]
HW.hw_destroy.argtypes = [C.c_void_p]
HW.hw_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
HW.hw_set_neighbours.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
HW.hw_reloc.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
HW.hw_reloc_line.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]

ctx = _lib.Context(_lib.default_params(), 640, 480, 1)
stream = side_stream()
rng = np.random.default_rng(99)


def vector(n_ids, n, base=None):
    """about n distinct ids with L1-normalised weights; with `base`, half of them are base's"""
    ids = rng.integers(0, n_ids, n)
    if base is not None:
        ids = np.concatenate([rng.choice(base, len(base) // 2, replace=False), ids[:n // 2]])
    ids = np.unique(ids).astype(np.int32)
    w = rng.random(len(ids)) + 0.05
    return ids, w / w.sum()


rows = []
for n_kf in [int(x) for x in args.kfs.split(",")]:
    db = KeyFrameDatabase(NP, NL, context=ctx)
    hw = HW.hw_create(NP, NL)
    kfs = []
    t0 = time.perf_counter()
    for k in range(n_kf):
        p, l = vector(NP, args.words), vector(NL, args.line_words)
        kfs.append((p, l))
        assert db.add(p, l) == k
    t_add = time.perf_counter() - t0
    for k, (p, l) in enumerate(kfs):
        HW.hw_add(hw, p[0].ctypes.data, p[1].ctypes.data, len(p[0]), l[0].ctypes.data, l[1].ctypes.data, len(l[0]))
    nb = {k: list(range(k - 1, max(k - 11, -1), -1)) for k in range(n_kf)}
    for k, v in nb.items():
        a = np.array(v + [-1], np.int32)
        HW.hw_set_neighbours(hw, k, a.ctypes.data, len(v))
    print(f"{n_kf} key frames: {np.mean([len(p[0]) for p, _ in kfs]):.0f} point words of {NP}, {np.mean([len(l[0]) for _, l in kfs]):.0f} line words of {NL}; "
          f"olf_kfdb_add {1e3 * t_add / n_kf:.3f} ms per key frame", flush=True)
    next_id = [1]
    for Q in [int(x) for x in args.queries.split(",")]:
        src = rng.integers(0, n_kf, Q)
        qp = [vector(NP, args.words, kfs[j][0][0]) for j in src]
        ql = [vector(NL, args.line_words, kfs[j][1][0]) for j in src]
        # ---- tables on the device: CSR queries uploaded once, tables stay there
        csr, tabs, keep = [], [], []
        for bows in (qp, ql):
            off, ids, vals = bow_csr(bows)
            d = (torch.from_numpy(ids).cuda(), torch.from_numpy(vals).cuda())
            t = (torch.empty(Q * n_kf, dtype=torch.int32, device="cuda"), torch.empty(Q * n_kf, dtype=torch.int32, device="cuda"),
                 torch.empty(Q * n_kf, dtype=torch.float64, device="cuda"))
            keep.append((off, d, t))
            csr.append(BowCsrC(off.ctypes.data, d[0].data_ptr(), d[1].data_ptr()))
            tabs.append(KfdbTablesC(*[x.data_ptr() for x in t]))
        run_p = lambda: check(lib().olf_kfdb_tables_dev(db._h, Q, C.byref(csr[0]), None, C.byref(tabs[0]), None, stream), "olf_kfdb_tables_dev")
        run_pl = lambda: check(lib().olf_kfdb_tables_dev(db._h, Q, C.byref(csr[0]), C.byref(csr[1]), C.byref(tabs[0]), C.byref(tabs[1]), stream), "olf_kfdb_tables_dev")
        t_tp, t_tpl = windows(run_p, True), windows(run_pl, True)
        common = keep[0][2][0].cpu().numpy()
        # ---- detect: host pointers in, candidate lists out
        # (the arrays are laid out once: converting Python lists for the C ABI is not what is timed)
        last = {}
        nb_off, nb_slots = _lists_csr(nb, n_kf)
        host_csr = [bow_csr(qp), bow_csr(ql)]
        hq = [BowCsrC(*[a.ctypes.data for a in c]) for c in host_csr]
        q_ids, q_np, q_nl = np.zeros(Q, np.int64), np.full(Q, 2000, np.int32), np.full(Q, 500, np.int32)
        c_off, c_slots = np.zeros(Q + 1, np.int32), np.zeros(Q * n_kf, np.int32)

        def detect(form):
            q_ids[:] = next_id[0] + np.arange(Q)
            next_id[0] += Q
            check(lib().olf_kfdb_detect(db._h, form, Q, q_ids.ctypes.data, C.byref(hq[0]), C.byref(hq[1]), q_np.ctypes.data, q_nl.ctypes.data, None, None, None,
                                        nb_off.ctypes.data, nb_slots.ctypes.data, c_off.ctypes.data, c_slots.ctypes.data, len(c_slots)), "olf_kfdb_detect")
            last[form] = [c_slots[c_off[i]:c_off[i + 1]].tolist() for i in range(Q)]

        t_d, t_dl = windows(lambda: detect(KFDB_RELOC), False), windows(lambda: detect(KFDB_RELOC_LINE), False)
        # ---- the host walk, one thread
        out = np.zeros(n_kf, np.int32)
        hw_last = {}

        def walk(line):
            res = []
            for i in range(Q):
                next_id[0] += 1
                if line:
                    n = HW.hw_reloc_line(hw, next_id[0], qp[i][0].ctypes.data, qp[i][1].ctypes.data, len(qp[i][0]), ql[i][0].ctypes.data, ql[i][1].ctypes.data,
                                         len(ql[i][0]), 2000, 500, out.ctypes.data)
                else:
                    n = HW.hw_reloc(hw, next_id[0], qp[i][0].ctypes.data, qp[i][1].ctypes.data, len(qp[i][0]), out.ctypes.data)
                res.append(out[:n].tolist())
            hw_last[line] = res

        t_w, t_wl = windows(lambda: walk(False), False), windows(lambda: walk(True), False)
        # (the two keep their own relocalisation scores across the timed calls, and a stale score can enter a sum: the lists are compared, not asserted)
        same = sum(a == b for a, b in zip(last[KFDB_RELOC], hw_last[False])), sum(a == b for a, b in zip(last[KFDB_RELOC_LINE], hw_last[True]))
        print(f"  Q = {Q}: common words per (query, key frame) {common.mean():.2f}, candidates per query {np.mean([len(c) for c in last[KFDB_RELOC]]):.1f}; "
              f"candidate lists equal to the host walk's: {same[0]} / {Q} plain, {same[1]} / {Q} with lines", flush=True)
        for tag, t in (("olf_kfdb_tables_dev points (HIP events)", t_tp), ("olf_kfdb_tables_dev points + lines (HIP events)", t_tpl),
                       ("olf_kfdb_detect reloc (host clock)", t_d), ("olf_kfdb_detect reloc with lines (host clock)", t_dl),
                       ("host walk reloc, one thread (host clock)", t_w), ("host walk reloc with lines, one thread (host clock)", t_wl)):
            print("    %-56s %9.3f ms per call, %8.3f ms per query (median of 5 windows of 10; min %.3f max %.3f)" % (tag, t[0], t[0] / Q, t[1], t[2]), flush=True)
        rows.append((n_kf, Q, t_tp[0], t_tpl[0], t_d[0], t_dl[0], t_w[0], t_wl[0]))
    HW.hw_destroy(hw)
    db.close()
print("\n| key frames | Q | tables_dev points | tables_dev points + lines | detect reloc | detect reloc + lines | host walk reloc | host walk reloc + lines |")
print("|---|---|---|---|---|---|---|---|")
for r in rows:
    print("| %d | %d | %s |" % (r[0], r[1], " | ".join("%.3f" % x for x in r[2:])))
print("(ms per call)")
ctx.close()
