"""KeyFrame::UpdateConnections (src/KeyFrame.cc:446-557) for a list of key frames against one snapshot of the map, and KeyFrame::UpdateBestCovisibles
(:216-235) for a batch of rows: olf_update_connections, olf_update_connections_batch_dev and olf_best_covisibles_batch_dev (include/orbline.h;
csrc/connections_batch.hip).

  UpdateConnections         host arrays in, per-key-frame lists out
  update_connections_batch  torch device tensors in and out, on torch's current stream; with the whole graph listed, its covis_offsets / covis_index are
                            kf_covis_offsets / kf_covis_index of a _lib.MapGraphC as they are
  best_covisibles_batch     rows of (key frame, weight) ordered as mvpOrderedConnectedKeyFrames, on the device

The snapshot is a localmap.MapGraph; only its observations, point flags and point slots are read, so one whose kf_covis is yet to be computed is built with
empty rows.  Convention C.16: ascending key-frame index stands for ascending KeyFrame* address."""
import ctypes as C
import numpy as np
from . import _lib
from ._lib import lib, ptr
from .localmap import MapGraph
from .matcher import _call_dev, _ctx, _dev, _new

OLF_COVIS_TH = 15                                                    # int th = 15, src/KeyFrame.cc:508


def UpdateConnections(graph, kf_list=None, th=OLF_COVIS_TH, context=None, capacities=None):
    """KeyFrame::UpdateConnections for every key frame of kf_list (None: all of the graph, in order): olf_update_connections.  capacities = (connected,
    ordered): the lengths of the two output lists (default: sized by a first call).  Returns a list with, per listed key frame, a dict of connected / weights
    (mConnectedKeyFrameWeights in ascending index), ordered / ordered_weights (mvpOrderedConnectedKeyFrames / mvOrderedWeights; ordered[0] is the parent
    candidate), kf_max (-1: none), w_max and n_counted.  A key frame with n_counted == 0 has empty lists: the reference keeps its old members there, which
    stays the caller's."""
    ctx = _ctx(context)
    lst = None if kf_list is None else np.ascontiguousarray(kf_list, dtype=np.int32).reshape(-1)
    n = graph.n_kf if lst is None else lst.shape[0]
    g = graph.c()
    nc, kmax, wmax = np.zeros(n, np.int32), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    offs = [np.zeros(n + 1, np.int32) for _ in range(2)]

    def run(caps):
        arr = [np.zeros(max(int(c), 1), np.int32) for c in caps for _ in range(2)]
        rc = lib().olf_update_connections(ctx.handle, C.byref(g), n, ptr(lst), int(th), ptr(nc), ptr(kmax), ptr(wmax), ptr(offs[0]), ptr(arr[0]), ptr(arr[1]),
                                          int(caps[0]), ptr(offs[1]), ptr(arr[2]), ptr(arr[3]), int(caps[1]))
        return rc, arr

    if capacities is None:                                           # a first call sizes the lists: the offsets are complete whatever the capacities
        rc, arr = run((0, 0))
        if rc == _lib.OLF_ERR_CAPACITY and any(int(o[n]) > 0 for o in offs):
            rc, arr = run([int(o[n]) for o in offs])
    else:
        rc, arr = run(capacities)
    _lib.check(rc, "olf_update_connections")
    (co, vo), cut = offs, lambda a, o, j: a[o[j]:o[j + 1]].copy()
    return [{"connected": cut(arr[0], co, j), "weights": cut(arr[1], co, j), "ordered": cut(arr[2], vo, j), "ordered_weights": cut(arr[3], vo, j),
             "kf_max": int(kmax[j]), "w_max": int(wmax[j]), "n_counted": int(nc[j])} for j in range(n)]


def update_connections_batch(graph, kf_list=None, n_list=None, th=OLF_COVIS_TH, capacities=(0, 0), out=None, context=None):
    """olf_update_connections_batch_dev on torch's current stream, without a synchronise.  graph: a MapGraph (its device copy is made once) or an
    _lib.MapGraphC of device pointers; kf_list: int32 device tensor [n_list], or None for the key frames 0 .. n_list - 1 (n_list defaults to the list's
    length, or to the graph's n_kf).  capacities = (connected, ordered): the lengths of the index / weight tensors.  Returns a dict of device tensors:
    n_counted, kf_max, w_max [n_list]; conn_offsets [n_list + 1] (always complete), conn_index, conn_weight; covis_offsets, covis_index, covis_weight.
    A list longer than its capacity is cut there and reported by the context's next synchronize() / poll_status()."""
    import torch
    ctx = _ctx(context)
    g = graph.c_dev() if isinstance(graph, MapGraph) else graph
    n = int(n_list) if n_list is not None else int(kf_list.shape[0]) if kf_list is not None else int(g.n_kf)
    if out is None:
        out = {}
    for k, c in zip(("conn", "covis"), capacities):
        out.setdefault(k + "_offsets", _new((n + 1,)))
        out.setdefault(k + "_index", _new((max(int(c), 1),)))
        out.setdefault(k + "_weight", _new((max(int(c), 1),)))
    out.setdefault("n_counted", _new((n,)))
    out.setdefault("kf_max", _new((n,), -1))
    out.setdefault("w_max", _new((n,)))
    i32 = torch.int32
    _call_dev("olf_update_connections_batch_dev", ctx, C.byref(g), n, _dev(kf_list, i32, "kf_list"), int(th), _dev(out["n_counted"], i32, "n_counted"),
              _dev(out["kf_max"], i32, "kf_max"), _dev(out["w_max"], i32, "w_max"),
              _dev(out["conn_offsets"], i32, "conn_offsets"), _dev(out["conn_index"], i32, "conn_index"), _dev(out["conn_weight"], i32, "conn_weight"), int(capacities[0]),
              _dev(out["covis_offsets"], i32, "covis_offsets"), _dev(out["covis_index"], i32, "covis_index"), _dev(out["covis_weight"], i32, "covis_weight"),
              int(capacities[1]))
    return out


def best_covisibles_batch(conn_offsets, conn_index, conn_weight, n_rows=None, out=None, context=None):
    """olf_best_covisibles_batch_dev on torch's current stream: KeyFrame::UpdateBestCovisibles for every row of the CSR conn_offsets [n_rows + 1] / conn_index
    / conn_weight (int32 device tensors).  Returns a dict of covis_index, covis_weight: every row in descending weight and, among equal weights, descending
    index, at the same offsets."""
    import torch
    ctx = _ctx(context)
    n = int(conn_offsets.shape[0]) - 1 if n_rows is None else int(n_rows)
    if out is None:
        out = {}
    out.setdefault("covis_index", torch.zeros_like(conn_index))
    out.setdefault("covis_weight", torch.zeros_like(conn_weight))
    i32 = torch.int32
    _call_dev("olf_best_covisibles_batch_dev", ctx, n, _dev(conn_offsets, i32, "conn_offsets"), _dev(conn_index, i32, "conn_index"),
              _dev(conn_weight, i32, "conn_weight"), _dev(out["covis_index"], i32, "covis_index"), _dev(out["covis_weight"], i32, "covis_weight"))
    return out
