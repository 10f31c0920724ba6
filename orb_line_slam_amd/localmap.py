"""Tracking::UpdateLocalMap (src/Tracking.cc:2028-2205) for a batch of frames against one snapshot of the map: olf_update_local_map and
olf_update_local_map_batch_dev (include/orbline.h; csrc/localmap_batch.hip).

  MapGraph                the snapshot (olf_map_graph): observations, bad flags, every key frame's point / line slots, ordered covisibility lists,
                          children and parents, as CSR arrays built from plain lists
  UpdateLocalMap          host arrays in, per-frame lists out
  update_local_map_batch  torch device tensors in and out, on torch's current stream; its point and line lists are list_offsets / list_index of
                          matcher.LocalMapDev / matcher.LocalLineMapDev as they are

Key frames, map points and map lines are numbered by the caller.  Convention C.16: ascending key-frame index stands for ascending KeyFrame* address, the
iteration order of the reference's std::map<KeyFrame*,int> and std::set<KeyFrame*>.
"""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import lib, ptr
from .matcher import _call_dev, _ctx, _dev, _new

OLF_LOCALMAP_MAX_KF = 8192


def _csr(rows, what):
    """(offsets [n + 1], index) int32 of a list of integer rows"""
    rows = [np.asarray(r, dtype=np.int64).reshape(-1) for r in rows]
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    if off[-1] > 0x7fffffff:
        raise ValueError(f"{what}: more than 2^31 entries")
    idx = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    if idx.size and (idx.min() < -0x80000000 or idx.max() > 0x7fffffff):
        raise ValueError(f"{what}: an index does not fit 32 bits")
    return off.astype(np.int32), np.ascontiguousarray(idx, dtype=np.int32)


def _flags(a, n, what):
    a = np.ascontiguousarray(np.asarray(a).astype(bool), dtype=np.uint8).reshape(-1)
    if a.shape[0] != n:
        raise ValueError(f"{what}: {n} flags expected, {a.shape[0]} given")
    return a


class MapGraph:
    """olf_map_graph from plain Python / numpy lists.
      mp_obs   [n_mp] rows: the key frames of MapPoint::GetObservations()          mp_bad [n_mp], kf_bad [n_kf], ml_bad [n_ml]: isBad()
      kf_mp    [n_kf] rows: GetMapPointMatches() in slot order, negative = NULL     kf_ml  [n_kf] rows, the same for GetMapLineMatches() (None: no lines)
      kf_covis [n_kf] rows: GetVectorCovisibleKeyFrames() in its order              kf_children [n_kf] rows: GetChilds() (any order: sorted here, C.16)
      kf_parent [n_kf]: GetParent(), -1 = none
    Raises ValueError for rows of the wrong number, a point / line / key-frame index outside the graph (NULL slots and parent -1 excepted), a key frame
    listed twice among one key frame's children, or more than OLF_LOCALMAP_MAX_KF key frames."""

    def __init__(self, mp_obs, mp_bad, kf_bad, kf_mp, kf_covis, kf_children, kf_parent, kf_ml=None, ml_bad=None):
        self.n_kf, self.n_mp = len(kf_bad), len(mp_bad)
        self.n_ml = 0 if ml_bad is None else len(ml_bad)
        if self.n_kf > OLF_LOCALMAP_MAX_KF:
            raise ValueError(f"MapGraph: more than OLF_LOCALMAP_MAX_KF = {OLF_LOCALMAP_MAX_KF} key frames")
        if (kf_ml is None) != (ml_bad is None):
            raise ValueError("MapGraph: kf_ml and ml_bad come together")
        for rows, n, what in ((mp_obs, self.n_mp, "mp_obs"), (kf_mp, self.n_kf, "kf_mp"), (kf_covis, self.n_kf, "kf_covis"), (kf_children, self.n_kf, "kf_children"),
                              (kf_ml if kf_ml is not None else [()] * self.n_kf, self.n_kf, "kf_ml")):
            if len(rows) != n:
                raise ValueError(f"MapGraph: {what}: {n} rows expected, {len(rows)} given")
        self.mp_bad, self.kf_bad = _flags(mp_bad, self.n_mp, "mp_bad"), _flags(kf_bad, self.n_kf, "kf_bad")
        self.ml_bad = None if ml_bad is None else _flags(ml_bad, self.n_ml, "ml_bad")
        self.mp_obs_offsets, self.mp_obs_kf = _csr(mp_obs, "mp_obs")
        self.kf_mp_offsets, self.kf_mp_index = _csr(kf_mp, "kf_mp")
        self.kf_ml_offsets, self.kf_ml_index = (None, None) if kf_ml is None else _csr(kf_ml, "kf_ml")
        self.kf_covis_offsets, self.kf_covis_index = _csr(kf_covis, "kf_covis")
        for k, r in enumerate(kf_children):
            if len(set(int(v) for v in r)) != len(r):
                raise ValueError(f"MapGraph: key frame {k} lists a child twice")
        self.kf_child_offsets, self.kf_child_index = _csr([sorted(int(v) for v in r) for r in kf_children], "kf_children")
        self.kf_parent = np.ascontiguousarray(np.asarray(kf_parent, dtype=np.int64).reshape(-1))
        if self.kf_parent.shape[0] != self.n_kf:
            raise ValueError(f"MapGraph: kf_parent: {self.n_kf} entries expected")
        for a, n, lo, what in ((self.mp_obs_kf, self.n_kf, 0, "mp_obs"), (self.kf_covis_index, self.n_kf, 0, "kf_covis"), (self.kf_child_index, self.n_kf, 0, "kf_children"),
                               (self.kf_parent, self.n_kf, -1, "kf_parent")):
            if a.size and (a.min() < lo or a.max() >= n):
                raise ValueError(f"MapGraph: {what}: a key-frame index outside [0, {n})")
        self.kf_parent = self.kf_parent.astype(np.int32)
        if self.kf_mp_index.size and self.kf_mp_index.max() >= self.n_mp:
            raise ValueError(f"MapGraph: kf_mp: a map-point index outside the map of {self.n_mp}")
        if kf_ml is not None and self.kf_ml_index.size and self.kf_ml_index.max() >= self.n_ml:
            raise ValueError(f"MapGraph: kf_ml: a map-line index outside the map of {self.n_ml}")
        self._dev = None

    _ARRAYS = ("mp_obs_offsets", "mp_obs_kf", "mp_bad", "ml_bad", "kf_bad", "kf_mp_offsets", "kf_mp_index", "kf_ml_offsets", "kf_ml_index", "kf_covis_offsets",
               "kf_covis_index", "kf_child_offsets", "kf_child_index", "kf_parent")

    def c(self):
        """olf_map_graph over the host arrays"""
        g = _lib.MapGraphC()
        g.n_kf, g.n_mp, g.n_ml = self.n_kf, self.n_mp, self.n_ml
        for k in self._ARRAYS:
            setattr(g, k, ptr(getattr(self, k)))
        return g

    def c_dev(self):
        """olf_map_graph over device copies of the arrays (torch tensors, made once and kept)"""
        import torch
        if self._dev is None:
            self._dev = {k: None if getattr(self, k) is None else torch.from_numpy(getattr(self, k)).cuda() for k in self._ARRAYS}
        g = _lib.MapGraphC()
        g.n_kf, g.n_mp, g.n_ml = self.n_kf, self.n_mp, self.n_ml
        for k, t in self._dev.items():
            setattr(g, k, None if t is None else t.data_ptr())
        return g


def _rows(a, n_frames, cap, what):
    """[n_frames, cap] int32 from rows of at most cap values each (padded with -1)"""
    out = np.full((n_frames, cap), -1, np.int32)
    if len(a) != n_frames:
        raise ValueError(f"{what}: {n_frames} rows expected")
    for j, r in enumerate(a):
        r = np.asarray(r, dtype=np.int32).reshape(-1)
        if r.shape[0] > cap:
            raise ValueError(f"{what}: row {j} holds more than the context's capacity of {cap}")
        out[j, :r.shape[0]] = r
    return out


def UpdateLocalMap(graph, frame_mp, frame_ml=None, counts=None, lcounts=None, context=None, capacities=None):
    """Tracking::UpdateLocalMap for every frame of a batch: olf_update_local_map.  frame_mp: per frame mvpMapPoints as map-point indices (negative: none, or a
    temporal point), frame_ml the same for mvpMapLines (None: no lines held); counts / lcounts: N / N_l per frame (default: the rows' lengths).
    capacities = (key frames, points, lines) of the three output lists (default: sized by a first call).  Returns a list with, per frame, a dict of
    local_kfs, local_points, local_lines (int32 arrays in the reference's order), ref_kf (-1: none), n_voted, frame_mp and frame_ml (the rows with their bad
    entries cleared to -1).  A frame with n_voted == 0 has empty lists: the reference keeps the previous frame's there, which stays the caller's."""
    ctx = _ctx(context)
    nf = len(frame_mp)
    cap, lcap = ctx.orb_capacity, ctx.line_capacity
    if counts is None:
        counts = [len(r) for r in frame_mp]
    if lcounts is None and frame_ml is not None:
        lcounts = [len(r) for r in frame_ml]
    fmp = _rows(frame_mp, nf, cap, "frame_mp")
    fml = None if frame_ml is None else _rows(frame_ml, nf, lcap, "frame_ml")
    cnt = np.ascontiguousarray(counts, dtype=np.int32)
    lcnt = None if lcounts is None else np.ascontiguousarray(lcounts, dtype=np.int32)
    if cnt.shape != (nf,) or (lcnt is not None and lcnt.shape != (nf,)):
        raise ValueError("UpdateLocalMap: one count per frame expected")
    g = graph.c()
    ref, nv = np.full(nf, -1, np.int32), np.zeros(nf, np.int32)
    offs = [np.zeros(nf + 1, np.int32) for _ in range(3)]
    fmp_out, fml_out = np.empty_like(fmp), None if fml is None else np.empty_like(fml)

    def run(caps):
        idx = [np.zeros(max(int(c), 1), np.int32) for c in caps]
        rc = lib().olf_update_local_map(ctx.handle, C.byref(g), nf, 1, ptr(cnt), ptr(lcnt), ptr(fmp), ptr(fml), ptr(fmp_out), ptr(fml_out), ptr(ref), ptr(nv),
                                        ptr(offs[0]), ptr(idx[0]), int(caps[0]), ptr(offs[1]), ptr(idx[1]), int(caps[1]), ptr(offs[2]), ptr(idx[2]), int(caps[2]))
        return rc, idx

    if capacities is None:                                           # a first call sizes the lists: the offsets are complete whatever the capacities
        rc, idx = run((0, 0, 0))
        if rc == _lib.OLF_ERR_CAPACITY and any(int(o[nf]) > 0 for o in offs):
            rc, idx = run([int(o[nf]) for o in offs])
    else:
        rc, idx = run(capacities)
    _lib.check(rc, "olf_update_local_map")
    out = []
    for j in range(nf):
        out.append({"local_kfs": idx[0][offs[0][j]:offs[0][j + 1]].copy(), "local_points": idx[1][offs[1][j]:offs[1][j + 1]].copy(),
                    "local_lines": idx[2][offs[2][j]:offs[2][j + 1]].copy(), "ref_kf": int(ref[j]), "n_voted": int(nv[j]),
                    "frame_mp": fmp_out[j, :cnt[j]].copy(), "frame_ml": None if fml is None else fml_out[j, :lcnt[j]].copy()})
    return out


def update_local_map_batch(graph, n_frames, frame_mp, counts=None, frame_ml=None, lcounts=None, img_stride=1, capacities=(0, 0, 0), out=None, inplace=False,
                           context=None):
    """olf_update_local_map_batch_dev on torch's current stream, without a synchronise.  graph: a MapGraph (its device copy is made once) or an
    _lib.MapGraphC of device pointers; frame_mp int32 [n_frames, orb capacity], frame_ml int32 [n_frames, line capacity] or None; counts / lcounts int32 in
    the extractor's layout with img_stride (None: every row is full).  capacities = (key frames, points, lines): the lengths of the three index tensors.
    Returns a dict of device tensors: kf_offsets / kf_index, mp_offsets / mp_index, ml_offsets / ml_index (the offsets [n_frames + 1], always complete),
    ref_kf, n_voted [n_frames], frame_mp, frame_ml (the cleaned rows; the inputs themselves with inplace=True).  mp_offsets / mp_index are list_offsets /
    list_index of a matcher.LocalMapDev, ml_offsets / ml_index those of a matcher.LocalLineMapDev.  A list longer than its capacity is cut there and
    reported by the context's next synchronize() / poll_status()."""
    import torch
    ctx = _ctx(context)
    nf = int(n_frames)
    g = graph.c_dev() if isinstance(graph, MapGraph) else graph
    if out is None:
        out = {}
    for k, c in zip(("kf", "mp", "ml"), capacities):
        out.setdefault(k + "_offsets", _new((nf + 1,)))
        out.setdefault(k + "_index", _new((max(int(c), 1),)))
    out.setdefault("ref_kf", _new((nf,), -1))
    out.setdefault("n_voted", _new((nf,)))
    out.setdefault("frame_mp", frame_mp if inplace else torch.empty_like(frame_mp))
    out.setdefault("frame_ml", None if frame_ml is None else frame_ml if inplace else torch.empty_like(frame_ml))
    i32 = torch.int32
    _call_dev("olf_update_local_map_batch_dev", ctx, C.byref(g), nf, int(img_stride), _dev(counts, i32, "counts"), _dev(lcounts, i32, "lcounts"),
              _dev(frame_mp, i32, "frame_mp"), _dev(frame_ml, i32, "frame_ml"), _dev(out["frame_mp"], i32, "frame_mp out"), _dev(out["frame_ml"], i32, "frame_ml out"),
              _dev(out["ref_kf"], i32, "ref_kf"), _dev(out["n_voted"], i32, "n_voted"),
              _dev(out["kf_offsets"], i32, "kf_offsets"), _dev(out["kf_index"], i32, "kf_index"), int(capacities[0]),
              _dev(out["mp_offsets"], i32, "mp_offsets"), _dev(out["mp_index"], i32, "mp_index"), int(capacities[1]),
              _dev(out["ml_offsets"], i32, "ml_offsets"), _dev(out["ml_index"], i32, "ml_index"), int(capacities[2]))
    return out
