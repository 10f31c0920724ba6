"""KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) on the GPU: place recognition for a batch of frames.

    db = KeyFrameDatabase(voc, voc_l, context=ctx)               # or the vocabularies' sizes as ints
    slot = db.add(kf_bow, kf_bow_l)                              # KeyFrameDatabase::add; a key frame is its slot from here on
    cands = db.DetectRelocalizationCandidates([Query(mnId=7, bow=f.bow), ...], neighbours)

A BoW vector is a {word id: value} dict (what ORBVocabulary.transform returns) or an (ids, vals) pair in ascending id order.  A query is a Query;
`neighbours` gives GetBestCovisibilityKeyFrames(10) of every slot in order, as a {slot: [slots]} dict or a list indexed by slot (None or a negative
entry: a neighbour that is not in the database).  The covisibility graph and isBad() stay with the caller; the selection does not.  The Detect members
take one query or a list (the list is the reference applied to the queries one after the other) and return slots in the reference's order.
"""
import ctypes as C
from dataclasses import dataclass, field
import numpy as np
from ._lib import BowCsrC, KfdbTablesC, KFDB_LOOP, KFDB_LOOP_LINE, KFDB_RELOC, KFDB_RELOC_LINE, check, lib, ptr


@dataclass
class Query:
    """what a Detect member reads of its KeyFrame* / Frame*: mnId, mBowVec, mBowVec_l, N, N_l and (loop forms) GetConnectedKeyFrames() as slots"""
    mnId: int
    bow: object
    bow_l: object = None
    N: int = 0
    N_l: int = 0
    connected: tuple = field(default_factory=tuple)


def bow_arrays(bow):
    """(ids int32, vals float64) of a BoW vector in ascending id order"""
    if bow is None:
        return np.zeros(0, np.int32), np.zeros(0, np.float64)
    if isinstance(bow, dict):
        ids = np.fromiter(sorted(bow), np.int32, len(bow))
        return ids, np.array([bow[int(i)] for i in ids], np.float64)
    ids, vals = bow
    return np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(vals, np.float64)


def bow_csr(bows):
    """(off int32 [n + 1], ids, vals) of a list of BoW vectors"""
    arrs = [bow_arrays(b) for b in bows]
    off = np.zeros(len(arrs) + 1, np.int32)
    off[1:] = np.cumsum([len(a[0]) for a in arrs])
    ids = np.concatenate([a[0] for a in arrs]) if arrs else np.zeros(0, np.int32)
    vals = np.concatenate([a[1] for a in arrs]) if arrs else np.zeros(0, np.float64)
    return off, np.ascontiguousarray(ids, np.int32), np.ascontiguousarray(vals, np.float64)


def _lists_csr(lists, n):
    """n lists of slots as (off [n + 1], slots); None and missing entries count as -1 / empty"""
    off, flat = np.zeros(n + 1, np.int32), []
    for i in range(n):
        row = (lists.get(i, ()) if isinstance(lists, dict) else (lists[i] if lists is not None and i < len(lists) else ())) or ()
        flat.extend(-1 if v is None else int(v) for v in row)
        off[i + 1] = len(flat)
    return off, np.array(flat + [-1], np.int32)[:len(flat)]          # (never a null pointer, even when empty)


def _n_words(voc):
    return int(voc) if isinstance(voc, (int, np.integer)) else (0 if voc is None else voc.size())


def _scoring(voc):
    return 0 if voc is None or isinstance(voc, (int, np.integer)) else voc.info()["scoring"]


class KeyFrameDatabase:
    def __init__(self, voc, voc_l=None, context=None, scoring=None, scoring_l=None):
        """KeyFrameDatabase(const ORBVocabulary&[, const LineVocabulary&]), src/KeyFrameDatabase.cc:33-44.  context None: a database without a device
        copy (add / erase / clear / select only)."""
        self._h = C.c_void_p()
        self._context = context
        check(lib().olf_kfdb_create(context.handle if context is not None else None, _n_words(voc), _n_words(voc_l),
                                    _scoring(voc) if scoring is None else int(scoring), _scoring(voc_l) if scoring_l is None else int(scoring_l),
                                    C.byref(self._h)), "olf_kfdb_create")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().olf_kfdb_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- KeyFrameDatabase::add / erase / clear, :46-98
    def add(self, bow, bow_l=None):
        (ip, vp), (il, vl) = bow_arrays(bow), bow_arrays(bow_l)
        slot = C.c_int32()
        check(lib().olf_kfdb_add(self._h, ptr(ip), ptr(vp), len(ip), ptr(il), ptr(vl), len(il), C.byref(slot)), "olf_kfdb_add")
        return slot.value

    def erase(self, slot):
        check(lib().olf_kfdb_erase(self._h, int(slot)), "olf_kfdb_erase")

    def clear(self):
        check(lib().olf_kfdb_clear(self._h), "olf_kfdb_clear")

    def size(self):
        """(slots handed out since the last clear, slots not erased)"""
        a, b = C.c_int32(), C.c_int32()
        check(lib().olf_kfdb_size(self._h, C.byref(a), C.byref(b)), "olf_kfdb_size")
        return a.value, b.value

    def state(self):
        """mRelocScore, mRelocScore_l, mRelocScore_pl of every slot: the members that survive a query"""
        n = self.size()[0]
        s = [np.zeros(n, np.float32) for _ in range(3)]
        check(lib().olf_kfdb_state(self._h, ptr(s[0]), ptr(s[1]), ptr(s[2])), "olf_kfdb_state")
        return dict(zip(("mRelocScore", "mRelocScore_l", "mRelocScore_pl"), s))

    # ---- the device half
    def tables(self, bows, bows_l=None):
        """olf_kfdb_tables_dev for a list of query vectors: {"common", "first", "score"} numpy tables [Q][slots] of the point vocabulary, and of the
        line vocabulary when bows_l is given"""
        import torch
        from .matcher import _torch_stream
        n, Q = self.size()[0], len(bows)
        keep, csr, tabs = [], [], []
        for b in (bows, bows_l):
            if b is None:
                csr.append(None); tabs.append(None)
                continue
            off, ids, vals = bow_csr(b)
            d_ids, d_vals = torch.from_numpy(np.append(ids, np.int32(0))).cuda(), torch.from_numpy(np.append(vals, 0.0)).cuda()     # (never empty: no null pointer)
            t = (torch.empty(Q * n + 1, dtype=torch.int32, device="cuda"), torch.empty(Q * n + 1, dtype=torch.int32, device="cuda"),
                 torch.empty(Q * n + 1, dtype=torch.float64, device="cuda"))
            keep.append((off, d_ids, d_vals))
            csr.append(BowCsrC(off.ctypes.data, d_ids.data_ptr(), d_vals.data_ptr()))
            tabs.append((KfdbTablesC(*[x.data_ptr() for x in t]), t))
        with _torch_stream() as s:
            check(lib().olf_kfdb_tables_dev(self._h, Q, C.byref(csr[0]), C.byref(csr[1]) if csr[1] else None, C.byref(tabs[0][0]),
                                            C.byref(tabs[1][0]) if tabs[1] else None, s), "olf_kfdb_tables_dev")
        torch.cuda.synchronize()
        out = [dict(zip(("common", "first", "score"), (x[:Q * n].cpu().numpy().reshape(Q, n) for x in t[1]))) if t else None for t in tabs]
        return out[0] if bows_l is None else tuple(out)

    def score_pairs(self, pairs, line=False, queries=None):
        """olf_bow_score_pairs_dev: L1 scores of (slot, slot) pairs, or of (query, slot) pairs when a list of query vectors is given"""
        import torch
        from .matcher import _torch_stream
        p = torch.from_numpy(np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)).cuda()
        n_pairs = len(p)
        p = torch.cat([p, torch.zeros(1, 2, dtype=torch.int32, device="cuda")])
        out = torch.empty(n_pairs + 1, dtype=torch.float64, device="cuda")
        csr, nq = None, 0
        if queries is not None:
            off, ids, vals = bow_csr(queries)
            keep = [torch.from_numpy(np.append(a, a.dtype.type(0))).cuda() for a in (off, ids, vals)]
            csr, nq = BowCsrC(*[a.data_ptr() for a in keep]), len(queries)
        with _torch_stream() as s:
            check(lib().olf_bow_score_pairs_dev(self._h, int(bool(line)), n_pairs, p.data_ptr(), C.byref(csr) if csr else None, nq, out.data_ptr(), s),
                  "olf_bow_score_pairs_dev")
        torch.cuda.synchronize()
        return out[:n_pairs].cpu().numpy()

    # ---- the host half
    def _query_args(self, form, queries, minScore, neighbours):
        loop, line = form in (KFDB_LOOP, KFDB_LOOP_LINE), form in (KFDB_LOOP_LINE, KFDB_RELOC_LINE)
        Q, n = len(queries), self.size()[0]
        ids = np.array([q.mnId for q in queries], np.int64)
        npts = np.array([q.N for q in queries], np.int32) if line else None
        nlin = np.array([q.N_l for q in queries], np.int32) if line else None
        ms = np.ascontiguousarray(np.broadcast_to(np.asarray(minScore, np.float32), (Q,))) if loop else None
        conn = _lists_csr([q.connected for q in queries], Q) if loop else (None, None)
        nb = _lists_csr(neighbours, n)
        return Q, n, ids, npts, nlin, ms, conn, nb

    def select(self, form, queries, tables, tables_l=None, minScore=0.0, neighbours=None):
        """olf_kfdb_select: the candidate lists of `queries` from host tables; updates the database's per-slot state"""
        Q, n, ids, npts, nlin, ms, conn, nb = self._query_args(form, queries, minScore, neighbours)
        tc = []
        for t in (tables, tables_l):
            if t is None:
                tc.append(None)
                continue
            arrs = (np.ascontiguousarray(t["common"], np.int32), np.ascontiguousarray(t["first"], np.int32), np.ascontiguousarray(t["score"], np.float64))
            tc.append((KfdbTablesC(*[a.ctypes.data for a in arrs]), arrs))
        off, cand = np.zeros(Q + 1, np.int32), np.zeros(max(Q * n, 1), np.int32)
        check(lib().olf_kfdb_select(self._h, form, Q, ptr(ids), ptr(npts), ptr(nlin), ptr(ms), ptr(conn[0]), ptr(conn[1]), ptr(nb[0]), ptr(nb[1]), n,
                                    C.byref(tc[0][0]) if tc[0] else None, C.byref(tc[1][0]) if tc[1] else None, ptr(off), ptr(cand), len(cand)),
              "olf_kfdb_select")
        return [cand[off[q]:off[q + 1]].tolist() for q in range(Q)]

    def detect(self, form, queries, minScore=0.0, neighbours=None):
        """olf_kfdb_detect: tables on the device, download, select"""
        Q, n, ids, npts, nlin, ms, conn, nb = self._query_args(form, queries, minScore, neighbours)
        line = form in (KFDB_LOOP_LINE, KFDB_RELOC_LINE)
        qp = bow_csr([q.bow for q in queries])
        ql = bow_csr([q.bow_l for q in queries]) if line else None
        cp = BowCsrC(*[a.ctypes.data for a in qp])
        cl = BowCsrC(*[a.ctypes.data for a in ql]) if line else None
        off, cand = np.zeros(Q + 1, np.int32), np.zeros(max(Q * n, 1), np.int32)
        check(lib().olf_kfdb_detect(self._h, form, Q, ptr(ids), C.byref(cp), C.byref(cl) if cl else None, ptr(npts), ptr(nlin), ptr(ms), ptr(conn[0]),
                                    ptr(conn[1]), ptr(nb[0]), ptr(nb[1]), ptr(off), ptr(cand), len(cand)), "olf_kfdb_detect")
        return [cand[off[q]:off[q + 1]].tolist() for q in range(Q)]

    def _detect(self, form, query, minScore, neighbours):
        one = isinstance(query, Query)
        out = self.detect(form, [query] if one else list(query), minScore, neighbours)
        return out[0] if one else out

    # ---- the reference's members
    def DetectLoopCandidates(self, pKF, minScore, neighbours=None):
        """vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore), :107-228; minScore: one value or one per query"""
        return self._detect(KFDB_LOOP, pKF, minScore, neighbours)

    def DetectLoopCandidatesWithLine(self, pKF, minScore, neighbours=None):
        """:230-400"""
        return self._detect(KFDB_LOOP_LINE, pKF, minScore, neighbours)

    def DetectRelocalizationCandidates(self, F, neighbours=None):
        """:402-512"""
        return self._detect(KFDB_RELOC, F, 0.0, neighbours)

    def DetectRelocalizationCandidatesWithLine(self, F, neighbours=None):
        """:514-667"""
        return self._detect(KFDB_RELOC_LINE, F, 0.0, neighbours)
