"""LocalMapping::KeyFrameCulling (src/LocalMapping.cc:632-696), LocalMapping::MapPointCulling (:170-205) and KeyFrame::TrackedMapPoints / TrackedMapLines
(src/KeyFrame.cc:328-353, 407-432) against one snapshot of the map: the olf_keyframe_culling*, olf_tracked_map_points* and olf_map_point_culling* entries
(include/orbline.h; csrc/culling_batch.hip, culling_host.cpp).

  CullView                       what KeyFrameCulling reads beyond a localmap.MapGraph (olf_cull_view), from plain lists
  keyframe_culling_tables_batch  the data-parallel tables, torch device tensors in and out, on torch's current stream
  keyframe_culling_replay        the sequential rest on the host, from the tables as numpy arrays
  KeyFrameCulling                host arrays in, the reference's decisions in list order out (tables, then replay)
  tracked_map_points_batch       device tensors; kf_list may be ref_kf of localmap.update_local_map_batch as it is, its -1 included
  TrackedMapPoints               host arrays
  map_point_culling              device tensors: one action per recent map point
  MapPointCulling                host arrays

KeyFrameCulling is not a pure function of the snapshot: a culled key frame erases its observations, so a later key frame of the list can lose or gain
redundancy.  The tables say what every listed key frame sees in the map as it stands; the replay gives what the reference decides."""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import lib, ptr
from .localmap import MapGraph, _csr, _flags
from .matcher import _call_dev, _ctx, _dev, _new

KEPT, CULLED, TO_BE_ERASED = 0, 1, 2                                 # decision of KeyFrameCulling
KEEP, ERASE_BAD, BAD_RATIO, BAD_FEW_OBS, ERASE_AGED = range(5)       # action of MapPointCulling


def _parallel(rows, offsets, dtype, what):
    """the rows of a per-entry array parallel to the CSR `offsets`, flattened"""
    if len(rows) != offsets.shape[0] - 1:
        raise ValueError(f"CullView: {what}: {offsets.shape[0] - 1} rows expected, {len(rows)} given")
    rows = [np.asarray(r, dtype=dtype).reshape(-1) for r in rows]
    for k, r in enumerate(rows):
        if r.shape[0] != offsets[k + 1] - offsets[k]:
            raise ValueError(f"CullView: {what}: row {k} holds {r.shape[0]} entries, the graph's row {offsets[k + 1] - offsets[k]}")
    return np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros(0, dtype), dtype=dtype)


class CullView:
    """olf_cull_view beside a MapGraph `graph`, from plain Python / numpy lists.
      mp_obs_slot [n_mp] rows parallel to mp_obs: the observer's feature index         mp_nobs [n_mp]: MapPoint::Observations()
      kf_slot_octave, kf_slot_depth, kf_slot_stereo [n_kf] rows parallel to kf_mp: mvKeysUn[i].octave, mvDepth[i], mvuRight[i] >= 0
      kf_th_depth [n_kf]: mThDepth                                                      kf_mode [n_kf]: 0 normal, 1 mbNotErase, 2 mnId == 0
    Raises ValueError for rows that do not match the graph's, an octave outside 0 .. 255 or a mode outside 0 .. 2."""

    def __init__(self, graph, mp_obs_slot, mp_nobs, kf_slot_octave, kf_slot_depth, kf_slot_stereo, kf_th_depth, kf_mode):
        self.n_kf, self.n_mp = graph.n_kf, graph.n_mp
        self.mp_obs_slot = _parallel(mp_obs_slot, graph.mp_obs_offsets, np.int32, "mp_obs_slot")
        octave = _parallel(kf_slot_octave, graph.kf_mp_offsets, np.int64, "kf_slot_octave")
        if octave.size and (octave.min() < 0 or octave.max() > 255):
            raise ValueError("CullView: kf_slot_octave: an octave outside 0 .. 255")
        self.kf_slot_octave = octave.astype(np.uint8)
        self.kf_slot_depth = _parallel(kf_slot_depth, graph.kf_mp_offsets, np.float32, "kf_slot_depth")
        self.kf_slot_stereo = (_parallel(kf_slot_stereo, graph.kf_mp_offsets, np.int64, "kf_slot_stereo") != 0).astype(np.uint8)
        self.mp_nobs = np.ascontiguousarray(mp_nobs, dtype=np.int32).reshape(-1)
        self.kf_th_depth = np.ascontiguousarray(kf_th_depth, dtype=np.float32).reshape(-1)
        mode = np.asarray(kf_mode, dtype=np.int64).reshape(-1)
        if mode.size and (mode.min() < 0 or mode.max() > 2):
            raise ValueError("CullView: kf_mode: a mode outside 0 .. 2")
        self.kf_mode = np.ascontiguousarray(mode, dtype=np.uint8)
        for a, n, what in ((self.mp_nobs, self.n_mp, "mp_nobs"), (self.kf_th_depth, self.n_kf, "kf_th_depth"), (self.kf_mode, self.n_kf, "kf_mode")):
            if a.shape[0] != n:
                raise ValueError(f"CullView: {what}: {n} entries expected, {a.shape[0]} given")
        self._dev = None

    _ARRAYS = ("mp_obs_slot", "mp_nobs", "kf_slot_octave", "kf_slot_depth", "kf_slot_stereo", "kf_th_depth", "kf_mode")

    def c(self):
        """olf_cull_view over the host arrays"""
        v = _lib.CullViewC()
        for k in self._ARRAYS:
            setattr(v, k, ptr(getattr(self, k)))
        return v

    def c_dev(self):
        """olf_cull_view over device copies of the arrays (torch tensors, made once and kept; an array without entries keeps an address)"""
        import torch
        if self._dev is None:
            pad = lambda a: a if a.size else np.zeros(1, a.dtype)
            self._dev = {k: torch.from_numpy(pad(getattr(self, k))).cuda() for k in self._ARRAYS}
        v = _lib.CullViewC()
        for k, t in self._dev.items():
            setattr(v, k, t.data_ptr())
        return v


def _graph_dev(graph):
    """olf_map_graph of device pointers in which an array without entries keeps an address (the culling entries require one)"""
    if not isinstance(graph, MapGraph):
        return graph
    import torch
    g = graph.c_dev()
    if not hasattr(graph, "_cull_pad"):
        graph._cull_pad = torch.zeros(4, dtype=torch.int32, device="cuda")
    for k in ("mp_obs_kf", "mp_bad", "kf_mp_index"):
        if not getattr(graph, k).size:
            setattr(g, k, graph._cull_pad.data_ptr())
    return g


def listed_slots(graph, kf_list=None, n_list=None):
    """the sum of the listed rows' lengths: the slot capacity keyframe_culling_tables_batch needs for this list"""
    off = graph.kf_mp_offsets.astype(np.int64)
    lst = np.arange(graph.n_kf if n_list is None else n_list) if kf_list is None else np.asarray(kf_list, dtype=np.int64).reshape(-1)
    lst = lst[(lst >= 0) & (lst < graph.n_kf)]
    return int((off[lst + 1] - off[lst]).sum())


def keyframe_culling_tables_batch(graph, view, kf_list=None, n_list=None, monocular=False, slot_capacity=0, out=None, context=None):
    """olf_keyframe_culling_tables_dev on torch's current stream, without a synchronise.  graph / view: a MapGraph and its CullView (their device copies are
    made once) or an _lib.MapGraphC / _lib.CullViewC of device pointers; kf_list: int32 device tensor [n_list], or None for the key frames 0 .. n_list - 1
    (n_list defaults to the list's length, or to the graph's n_kf).  slot_capacity: the length of the two per-slot tensors (listed_slots()).  Returns a dict of
    device tensors: n_mps, n_redundant (int32), redundant (uint8) [n_list]; row_offsets [n_list + 1] (always complete), slot_count (int32), slot_flags
    (uint8: bit 0 counted, bit 1 redundant).  Slots beyond slot_capacity are not written and are reported by the context's next synchronize() /
    poll_status()."""
    import torch
    ctx = _ctx(context)
    g = _graph_dev(graph)
    v = view.c_dev() if isinstance(view, CullView) else view
    n = int(n_list) if n_list is not None else int(kf_list.shape[0]) if kf_list is not None else int(g.n_kf)
    if out is None:
        out = {}
    out.setdefault("n_mps", _new((n,)))
    out.setdefault("n_redundant", _new((n,)))
    out.setdefault("redundant", _new((n,), dtype=torch.uint8))
    out.setdefault("row_offsets", _new((n + 1,)))
    out.setdefault("slot_count", _new((max(int(slot_capacity), 1),)))
    out.setdefault("slot_flags", _new((max(int(slot_capacity), 1),), dtype=torch.uint8))
    i32, u8 = torch.int32, torch.uint8
    _call_dev("olf_keyframe_culling_tables_dev", ctx, C.byref(g), C.byref(v), n, _dev(kf_list, i32, "kf_list"), int(bool(monocular)), _dev(out["n_mps"], i32, "n_mps"),
              _dev(out["n_redundant"], i32, "n_redundant"), _dev(out["redundant"], u8, "redundant"), _dev(out["row_offsets"], i32, "row_offsets"),
              _dev(out["slot_count"], i32, "slot_count"), _dev(out["slot_flags"], u8, "slot_flags"), int(slot_capacity))
    return out


def _list(kf_list, graph):
    lst = None if kf_list is None else np.ascontiguousarray(kf_list, dtype=np.int32).reshape(-1)
    return lst, graph.n_kf if lst is None else lst.shape[0]


def _replay_outputs(n, n_mp):
    return dict(decision=np.zeros(n, np.int32), n_mps=np.zeros(n, np.int32), n_redundant=np.zeros(n, np.int32), mp_nobs=np.zeros(n_mp, np.int32),
                mp_bad=np.zeros(n_mp, np.uint8), went_bad=np.zeros(n_mp, np.int32))


def keyframe_culling_replay(graph, view, kf_list, n_mps, n_redundant, row_offsets, slot_count, slot_flags):
    """olf_keyframe_culling_replay: the sequential rest of KeyFrameCulling on the host, no device.  graph / view: a MapGraph and its CullView; kf_list: the
    list (None: every key frame); the other arguments: the tables of keyframe_culling_tables_batch for that list as arrays.  Returns a dict of decision
    (0 kept, 1 culled, 2 mbToBeErased), n_mps, n_redundant (as the reference saw them at that moment) per listed key frame, mp_nobs, mp_bad (the final
    state of the points) and went_bad (the points that went bad, in order)."""
    lst, n = _list(kf_list, graph)
    tab = [np.ascontiguousarray(a, dtype=t).reshape(-1) for a, t in ((n_mps, np.int32), (n_redundant, np.int32), (row_offsets, np.int32), (slot_count, np.int32),
                                                                     (slot_flags, np.uint8))]
    if tab[0].shape[0] != n or tab[1].shape[0] != n or tab[2].shape[0] != n + 1 or tab[3].shape[0] < tab[2][-1] or tab[4].shape[0] < tab[2][-1]:
        raise ValueError("keyframe_culling_replay: the tables do not match the list")
    o, nb = _replay_outputs(n, graph.n_mp), C.c_int32(0)
    g, v = graph.c(), view.c()
    _lib.check(lib().olf_keyframe_culling_replay(C.byref(g), C.byref(v), n, ptr(lst), *(ptr(a) for a in tab), ptr(o["decision"]), ptr(o["n_mps"]), ptr(o["n_redundant"]),
                                                 ptr(o["mp_nobs"]), ptr(o["mp_bad"]), ptr(o["went_bad"]), C.addressof(nb)), "olf_keyframe_culling_replay")
    o["went_bad"] = o["went_bad"][:nb.value].copy()
    return o


def KeyFrameCulling(graph, view, kf_list=None, monocular=False, context=None):
    """LocalMapping::KeyFrameCulling over kf_list (GetVectorCovisibleKeyFrames() of the current key frame, in its order; None: every key frame of the graph):
    olf_keyframe_culling.  Returns the dict of keyframe_culling_replay and, beside it, table_n_mps, table_n_redundant and table_redundant: what every listed
    key frame sees in the map as it stands.  The caller runs SetBadFlag() on the key frames whose decision is not 0, in list order."""
    ctx = _ctx(context)
    lst, n = _list(kf_list, graph)
    o, nb = _replay_outputs(n, graph.n_mp), C.c_int32(0)
    o.update(table_n_mps=np.zeros(n, np.int32), table_n_redundant=np.zeros(n, np.int32), table_redundant=np.zeros(n, np.uint8))
    g, v = graph.c(), view.c()
    _lib.check(lib().olf_keyframe_culling(ctx.handle, C.byref(g), C.byref(v), n, ptr(lst), int(bool(monocular)), ptr(o["decision"]), ptr(o["n_mps"]),
                                          ptr(o["n_redundant"]), ptr(o["table_n_mps"]), ptr(o["table_n_redundant"]), ptr(o["table_redundant"]), ptr(o["mp_nobs"]),
                                          ptr(o["mp_bad"]), ptr(o["went_bad"]), C.addressof(nb)), "olf_keyframe_culling")
    o["went_bad"] = o["went_bad"][:nb.value].copy()
    return o


def tracked_map_points_batch(graph, mp_nobs, kf_list=None, ml_nobs=None, n_list=None, min_obs_points=0, min_obs_lines=0, out=None, context=None):
    """olf_tracked_map_points_batch_dev on torch's current stream, without a synchronise: KeyFrame::TrackedMapPoints(min_obs_points) and
    TrackedMapLines(min_obs_lines) of every listed key frame.  graph: a MapGraph or an _lib.MapGraphC of device pointers; mp_nobs / ml_nobs: int32 device
    tensors [n_mp] / [n_ml] (None where there is no observation test); kf_list: int32 device tensor, e.g. ref_kf of update_local_map_batch as it is (-1: no
    reference key frame, both counts 0), or None for the key frames 0 .. n_list - 1.  Returns a dict of n_points, n_lines [n_list]."""
    import torch
    ctx = _ctx(context)
    g = _graph_dev(graph)
    n = int(n_list) if n_list is not None else int(kf_list.shape[0]) if kf_list is not None else int(g.n_kf)
    if out is None:
        out = {}
    out.setdefault("n_points", _new((n,)))
    out.setdefault("n_lines", _new((n,)))
    i32 = torch.int32
    _call_dev("olf_tracked_map_points_batch_dev", ctx, C.byref(g), _dev(mp_nobs, i32, "mp_nobs"), _dev(ml_nobs, i32, "ml_nobs"), n, _dev(kf_list, i32, "kf_list"),
              int(min_obs_points), int(min_obs_lines), _dev(out["n_points"], i32, "n_points"), _dev(out["n_lines"], i32, "n_lines"))
    return out


def TrackedMapPoints(graph, mp_nobs, kf_list=None, ml_nobs=None, min_obs_points=0, min_obs_lines=0, context=None):
    """KeyFrame::TrackedMapPoints / TrackedMapLines of every listed key frame from host arrays: olf_tracked_map_points.  Returns (n_points, n_lines)."""
    ctx = _ctx(context)
    lst, n = _list(kf_list, graph)
    nobs = None if mp_nobs is None else np.ascontiguousarray(mp_nobs, dtype=np.int32).reshape(-1)
    lnobs = None if ml_nobs is None else np.ascontiguousarray(ml_nobs, dtype=np.int32).reshape(-1)
    if (nobs is not None and nobs.shape[0] != graph.n_mp) or (lnobs is not None and lnobs.shape[0] != graph.n_ml):
        raise ValueError("TrackedMapPoints: one observation count per map point / map line expected")
    n_points, n_lines = np.zeros(n, np.int32), np.zeros(n, np.int32)
    g = graph.c()
    _lib.check(lib().olf_tracked_map_points(ctx.handle, C.byref(g), ptr(nobs), ptr(lnobs), n, ptr(lst), int(min_obs_points), int(min_obs_lines), ptr(n_points),
                                            ptr(n_lines)), "olf_tracked_map_points")
    return n_points, n_lines


def map_point_culling(bad, found, visible, nobs, first_kf_id, current_kf_id, monocular=False, out=None, context=None):
    """olf_map_point_culling_dev on torch's current stream, without a synchronise: LocalMapping::MapPointCulling as one action per point of
    mlpRecentAddedMapPoints.  bad uint8, found / visible / nobs int32, first_kf_id int64: device tensors [n].  Returns the uint8 device tensor action [n]:
    0 keep, 1 erase from the list (bad), 2 SetBadFlag and erase (found ratio), 3 SetBadFlag and erase (few observations), 4 erase (aged)."""
    import torch
    ctx = _ctx(context)
    n = int(bad.shape[0])
    if out is None:
        out = _new((n,), dtype=torch.uint8)
    _call_dev("olf_map_point_culling_dev", ctx, n, _dev(bad, torch.uint8, "bad"), _dev(found, torch.int32, "found"), _dev(visible, torch.int32, "visible"),
              _dev(nobs, torch.int32, "nobs"), _dev(first_kf_id, torch.int64, "first_kf_id"), int(current_kf_id), int(bool(monocular)), _dev(out, torch.uint8, "action"))
    return out


def MapPointCulling(bad, found, visible, nobs, first_kf_id, current_kf_id, monocular=False, context=None):
    """LocalMapping::MapPointCulling from host arrays: olf_map_point_culling.  Returns the uint8 array of actions (map_point_culling)."""
    ctx = _ctx(context)
    bad = _flags(bad, len(bad), "bad")
    n = bad.shape[0]
    arr = [np.ascontiguousarray(a, dtype=t).reshape(-1) for a, t in ((found, np.int32), (visible, np.int32), (nobs, np.int32), (first_kf_id, np.int64))]
    if any(a.shape[0] != n for a in arr):
        raise ValueError("MapPointCulling: one entry per point expected in every array")
    action = np.zeros(n, np.uint8)
    _lib.check(lib().olf_map_point_culling(ctx.handle, n, ptr(bad), *(ptr(a) for a in arr), int(current_kf_id), int(bool(monocular)), ptr(action)), "olf_map_point_culling")
    return action
