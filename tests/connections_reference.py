"""KeyFrame::UpdateConnections (src/KeyFrame.cc:446-557) and KeyFrame::UpdateBestCovisibles (:216-235) restated line by line in Python: the oracle of
olf_update_connections*, olf_best_covisibles_batch_dev (tests/test_connections_cpu.py, tests/test_connections_gpu.py).

KFcounter and mConnectedKeyFrameWeights are dicts keyed by key-frame index and iterated in ascending key: convention C.16 lets ascending index
stand for the address order of std::map<KeyFrame*,int>.  vPairs is a list of (weight, index) tuples: Python's tuple order is std::pair's.  sort(vPairs)
followed by the push_front loop is a sort followed by a reversal.  Nothing here is vectorised or shared with the library's Python wrapper.  Parity unpinned:
the reference cannot be run here (its third-party libraries are not vendored), so every function follows the cited lines by reading."""


def update_connections(graph, kf, th=15):
    """UpdateConnections of key frame `kf` of a scene's graph() (mp_obs, mp_bad, kf_mp; kf_ml / ml_bad are walked as the reference walks them and change
    nothing).  Returns the dict orb_line_slam_amd.UpdateConnections returns for one key frame, as lists."""
    KFcounter = {}
    vpMP = graph["kf_mp"][kf]
    vpML = graph["kf_ml"][kf] if graph.get("kf_ml") is not None else []
    for pMP in vpMP:                                                 # :461-479
        if pMP < 0:
            continue
        if graph["mp_bad"][pMP]:
            continue
        for o in sorted(graph["mp_obs"][pMP]):
            if o == kf:
                continue
            KFcounter[o] = KFcounter.get(o, 0) + 1
    for pML in vpML:                                                 # :480-498
        if pML < 0:
            continue
        if graph["ml_bad"][pML]:
            continue
        pass                                                         # :496  // KFcounter[mit->first]++;
    if not KFcounter:                                                # :501
        return dict(connected=[], weights=[], ordered=[], ordered_weights=[], kf_max=-1, w_max=0, n_counted=0)
    nmax, pKFmax = 0, None
    vPairs = []
    for k in sorted(KFcounter):                                      # :512-524
        if KFcounter[k] > nmax:
            nmax, pKFmax = KFcounter[k], k
        if KFcounter[k] >= th:
            vPairs.append((KFcounter[k], k))
    if not vPairs:                                                   # :526-530
        vPairs.append((nmax, pKFmax))
    vPairs.sort()                                                    # :532
    lKFs, lWs = [], []
    for w, k in vPairs:                                              # :535-539
        lKFs.insert(0, k)
        lWs.insert(0, w)
    keys = sorted(KFcounter)
    return dict(connected=keys, weights=[KFcounter[k] for k in keys], ordered=lKFs, ordered_weights=lWs, kf_max=pKFmax, w_max=nmax, n_counted=len(KFcounter))


def update_connections_list(graph, kf_list=None, th=15):
    """every listed key frame (None: all, in order) against the graph as it stands"""
    n_kf = len(graph["kf_mp"])
    return [update_connections(graph, k, th) for k in (range(n_kf) if kf_list is None else kf_list)]


def update_best_covisibles(weights):
    """:216-235 on mConnectedKeyFrameWeights = {index: weight}; returns (mvpOrderedConnectedKeyFrames, mvOrderedWeights)"""
    vPairs = [(weights[k], k) for k in sorted(weights)]
    vPairs.sort()
    lKFs, lWs = [], []
    for w, k in vPairs:
        lKFs.insert(0, k)
        lWs.insert(0, w)
    return lKFs, lWs
