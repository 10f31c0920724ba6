"""A line-by-line restatement of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:632-696) with what it calls -- KeyFrame::SetBadFlag
(src/KeyFrame.cc:631-649), MapPoint::EraseObservation (src/MapPoint.cc:123-149), MapPoint::SetBadFlag (:163-180), KeyFrame::EraseMapPointMatch -- of
LocalMapping::MapPointCulling (:170-205) and of KeyFrame::TrackedMapPoints / TrackedMapLines (src/KeyFrame.cc:328-353, 407-432).  Plain Python loops over
the plain lists of a scene (tests/culling_scenes.py: CullScene.world()); nothing is vectorised and nothing is shared with the package.

A world `w` is a dict of lists: kf_mp / kf_oct / kf_depth / kf_stereo [n_kf][slots], th_depth, mode [n_kf], mp_obs [n_mp] rows of [key frame, slot] pairs,
mp_bad, mp_nobs [n_mp].  Malformed entries are left out as include/orbline.h says: a slot index >= n_mp, an observing key frame outside the graph, an
observation slot outside that key frame's row, a listed key frame outside the graph."""
import numpy as np

TH_OBS = 3                                                           # int nObs = 3; const int thObs = nObs, :647-648


def evaluate(w, kf, monocular):
    """the loop :651-691 for key frame kf against the world as it stands.  Returns nMPs, nRedundantObservations, the comparison of :693 and, per slot of the
    row, the uncapped number of qualifying observations and the flags (bit 0 counted, bit 1 redundant) -- what olf_keyframe_culling_tables_dev computes."""
    if not 0 <= kf < w["n_kf"]:
        return dict(n_mps=0, n_redundant=0, redundant=0, slot_count=[], slot_flags=[])
    vpMapPoints = w["kf_mp"][kf]
    nRedundantObservations = 0
    nMPs = 0
    slot_count, slot_flags = [0] * len(vpMapPoints), [0] * len(vpMapPoints)
    for i in range(len(vpMapPoints)):
        pMP = vpMapPoints[i]
        if pMP >= 0 and pMP < w["n_mp"]:                              # if(pMP)
            if not w["mp_bad"][pMP]:
                if not monocular:
                    if w["kf_depth"][kf][i] > w["th_depth"][kf] or w["kf_depth"][kf][i] < 0:
                        continue
                nMPs += 1
                scaleLevel = w["kf_oct"][kf][i]
                observations = [o for o in w["mp_obs"][pMP] if 0 <= o[0] < w["n_kf"] and (o[0] == kf or 0 <= o[1] < len(w["kf_mp"][o[0]]))]
                uncapped = 0
                for pKFi, idx in observations:
                    if pKFi == kf:
                        continue
                    if w["kf_oct"][pKFi][idx] <= scaleLevel + 1:
                        uncapped += 1
                slot_count[i], slot_flags[i] = uncapped, 1
                if w["mp_nobs"][pMP] > TH_OBS:
                    nObs = 0
                    for pKFi, idx in observations:
                        if pKFi == kf:
                            continue
                        scaleLeveli = w["kf_oct"][pKFi][idx]
                        if scaleLeveli <= scaleLevel + 1:
                            nObs += 1
                            if nObs >= TH_OBS:
                                break
                    if nObs >= TH_OBS:
                        nRedundantObservations += 1
                        slot_flags[i] = 3
    return dict(n_mps=nMPs, n_redundant=nRedundantObservations, redundant=int(float(nRedundantObservations) > 0.9 * float(nMPs)), slot_count=slot_count,
                slot_flags=slot_flags)


def status_bits(w, kf_list, monocular):
    """the status bits the tables raise for the list: 512 for a slot index >= n_mp, 4096 for a listed key frame outside the graph and for an observation of a
    counted slot (not the listed key frame's own) whose key frame is outside the graph or whose slot is outside that key frame's row"""
    bits = 0
    for kf in kf_list:
        if not 0 <= kf < w["n_kf"]:
            bits |= 4096
            continue
        for i, p in enumerate(w["kf_mp"][kf]):
            if p >= w["n_mp"]:
                bits |= 512
            if not 0 <= p < w["n_mp"] or w["mp_bad"][p]:
                continue
            if not monocular and (w["kf_depth"][kf][i] > w["th_depth"][kf] or w["kf_depth"][kf][i] < 0):
                continue
            for k, s in w["mp_obs"][p]:
                if k != kf and (not 0 <= k < w["n_kf"] or not 0 <= s < len(w["kf_mp"][k])):
                    bits |= 4096
    return bits


def tables(w, kf_list, monocular):
    """evaluate() of every listed key frame, each against the world as it stands, in the layout of olf_keyframe_culling_tables_dev"""
    rows = [evaluate(w, kf, monocular) for kf in kf_list]
    off = [0]
    for r in rows:
        off.append(off[-1] + len(r["slot_count"]))
    return dict(n_mps=[r["n_mps"] for r in rows], n_redundant=[r["n_redundant"] for r in rows], redundant=[r["redundant"] for r in rows], row_offsets=off,
                slot_count=[v for r in rows for v in r["slot_count"]], slot_flags=[v for r in rows for v in r["slot_flags"]])


# ---- the sequential simulation -------------------------------------------------------------------------------------------------------------------------------
def _mp_set_bad_flag(w, p, went_bad):
    """MapPoint::SetBadFlag, src/MapPoint.cc:163-180"""
    w["mp_bad"][p] = 1
    obs = w["mp_obs"][p]
    w["mp_obs"][p] = []
    for pKF, idx in obs:
        w["kf_mp"][pKF][idx] = -1                                    # pKF->EraseMapPointMatch(mit->second)
    went_bad.append(p)


def _mp_erase_observation(w, p, pKF, went_bad):
    """MapPoint::EraseObservation, src/MapPoint.cc:123-149"""
    bBad = False
    found = [o for o in w["mp_obs"][p] if o[0] == pKF]
    if found:                                                        # if(mObservations.count(pKF))
        idx = found[0][1]
        if w["kf_stereo"][pKF][idx]:                                 # pKF->mvuRight[idx]>=0
            w["mp_nobs"][p] -= 2
        else:
            w["mp_nobs"][p] -= 1
        w["mp_obs"][p].remove(found[0])
        if w["mp_nobs"][p] <= 2:
            bBad = True
    if bBad:
        _mp_set_bad_flag(w, p, went_bad)


def _kf_set_bad_flag(w, pKF, gone, went_bad):
    """KeyFrame::SetBadFlag, src/KeyFrame.cc:631-649 (the rest of it repairs the spanning tree).  Returns the decision: 0 mnId == 0, 2 mbToBeErased, 1 culled."""
    if w["mode"][pKF] == 2:
        return 0
    elif w["mode"][pKF] == 1:
        return 2
    for i in range(len(w["kf_mp"][pKF])):
        if w["kf_mp"][pKF][i] >= 0:
            _mp_erase_observation(w, w["kf_mp"][pKF][i], pKF, went_bad)
    gone.add(pKF)
    return 1


def keyframe_culling(world, kf_list, monocular):
    """LocalMapping::KeyFrameCulling over kf_list on a world that it changes as the reference changes the map (pass a copy).  The observation rows of the
    points that are bad at the start are cleared first: SetBadFlag cleared them when they went bad.  A key frame outside the graph, one of mode 2 and one
    that was culled earlier in the list give decision 0 and counts 0.  Returns decision, n_mps, n_redundant per listed key frame, the points that went bad in
    order and the final mp_nobs and mp_bad."""
    w = world
    for p in range(w["n_mp"]):
        if w["mp_bad"][p]:
            w["mp_obs"][p] = []
    decision, n_mps, n_red, went_bad, gone = [], [], [], [], set()
    for pKF in kf_list:
        if not 0 <= pKF < w["n_kf"] or w["mode"][pKF] == 2 or pKF in gone:      # if(pKF->mnId==0) continue
            decision.append(0); n_mps.append(0); n_red.append(0)
            continue
        e = evaluate(w, pKF, monocular)
        n_mps.append(e["n_mps"]); n_red.append(e["n_redundant"])
        if e["n_redundant"] > 0.9 * e["n_mps"]:
            decision.append(_kf_set_bad_flag(w, pKF, gone, went_bad))
        else:
            decision.append(0)
    return dict(decision=decision, n_mps=n_mps, n_redundant=n_red, went_bad=went_bad, mp_nobs=list(w["mp_nobs"]), mp_bad=[int(b) for b in w["mp_bad"]])


# ---- MapPointCulling ---------------------------------------------------------------------------------------------------------------------------------------
def _as_int(v):
    """(int) of an unsigned long"""
    v &= 0xffffffff
    return v - (1 << 32) if v & 0x80000000 else v


def map_point_culling(bad, found, visible, nobs, first_kf_id, current_kf_id, monocular):
    """LocalMapping::MapPointCulling, :170-205, as one action per point: 0 keep, 1 erase (bad), 2 SetBadFlag and erase (ratio), 3 SetBadFlag and erase (few
    observations), 4 erase (aged)"""
    nThObs = 2 if monocular else 3
    action = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(len(bad)):
            ratio = np.float32(found[i]) / np.float32(visible[i])   # static_cast<float>(mnFound)/mnVisible
            age = _as_int(int(current_kf_id)) - _as_int(int(first_kf_id[i]))
            if bad[i]:
                action.append(1)
            elif ratio < np.float32(0.25):
                action.append(2)
            elif age >= 2 and nobs[i] <= nThObs:
                action.append(3)
            elif age >= 3:
                action.append(4)
            else:
                action.append(0)
    return action


# ---- TrackedMapPoints / TrackedMapLines ------------------------------------------------------------------------------------------------------------------
def tracked(row, bad, nobs, minObs):
    """KeyFrame::TrackedMapPoints (src/KeyFrame.cc:328-353) over one row of slots; TrackedMapLines (:407-432) is the same loop over the line slots"""
    nPoints = 0
    bCheckObs = minObs > 0
    for i in range(len(row)):
        pMP = row[i]
        if pMP >= 0 and pMP < len(bad):
            if not bad[pMP]:
                if bCheckObs:
                    if nobs[pMP] >= minObs:
                        nPoints += 1
                else:
                    nPoints += 1
    return nPoints
