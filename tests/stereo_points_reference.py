"""Frame::ComputeStereoMatches (reference src/Frame.cc:702-876) restated line by line as sequential Python over np.float32 scalars -- a second
reference beside oracle/stereo_oracle.cpp, written from the reference source (line numbers below), not from the oracle or the kernels.

compute_stereo_matches() returns, besides mvuRight / mvDepth / the accepted SAD, what the scenes need to say WHY a key point ended as it did: the
chosen iR and bestDist, all 11 SADs, bestincR and a tag naming the gate that rejected it.  A SAD window or strip that would leave its level image
raises SceneError: the reference's rowRange / colRange throw there, so such a scene is not a valid input.  So does any right key point that passes a
left key point's gates with scaleduR0 < 10 on the left point's level, chosen or not: had it been the best, its strip would start left of column 0.

mutate= applies ONE named change to the restated code: the CPU tests show with it that the scenes would notice that mistake.
"""
import math
import numpy as np

f32 = np.float32
TH_HIGH, TH_LOW = 100, 50            # src/ORBmatcher.cc:39-40
INT_MAX = 2 ** 31 - 1

MUTATIONS = ("tie_last", "th_le", "oct_wide", "band_trunc", "u_open", "no_endu", "keep_edge_inc", "rint", "sad15", "median_lo", "thdist_le",
             "zero_disp_reject")

# the gate that ended a left key point (in the order of the code)
TAGS = ("no_row_cand", "maxU", "no_match", "endu", "edge_inc", "delta", "disparity", "median", "ok")

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


class SceneError(Exception):
    """the reference would read outside a pyramid level (cv::Mat::rowRange / colRange throw)"""


def hamming(a, b):
    return int(_POP[np.bitwise_xor(a, b)].sum())       # ORBmatcher::DescriptorDistance, src/ORBmatcher.cc:1795-1811


def c_round(v):
    """round(): half away from zero (v is a float32 value; v + 0.5 is exact in double)"""
    v = float(v)
    return f32(math.floor(v + 0.5) if v >= 0 else -math.floor(-v + 0.5))


def compute_stereo_matches(kpsL, descL, kpsR, descR, pyrL, pyrR, sf, inv_sf, bf, fx, mutate=None):
    assert mutate is None or mutate in MUTATIONS, mutate
    N = len(kpsL)
    mbf = f32(bf)
    mb = mbf / f32(fx)                                                      # src/Frame.cc:197
    uRight = np.full(N, -1.0, f32)                                          # :704
    depth = np.full(N, -1.0, f32)                                           # :705
    sad = np.full(N, -1, np.int32)
    out_iR = np.zeros(N, np.int64)
    out_dist = np.full(N, TH_HIGH, np.int32)
    out_sads = np.full((N, 11), -1, np.int64)
    out_inc = np.zeros(N, np.int32)
    tag = np.array(["ok"] * N, dtype="U12")
    if N == 0:                                                              # Frame::Frame returns before the call, :176-177
        return dict(uRight=uRight, depth=depth, sad=sad, iR=out_iR, bestDist=out_dist, sads=out_sads, bestinc=out_inc, tag=tag)
    rnd = (lambda v: f32(np.rint(f32(v)))) if mutate == "rint" else c_round

    thOrbDist = (TH_HIGH + TH_LOW) // 2                                     # :707
    nRows = pyrL[0].shape[0]                                                # :709
    vRowIndices = [[] for _ in range(nRows)]                                # :712
    Nr = len(kpsR)                                                          # :717
    for iR in range(Nr):                                                    # :719
        kpY = f32(kpsR["y"][iR])
        r = f32(2.0) * f32(sf[int(kpsR["octave"][iR])])                     # :723
        if mutate == "band_trunc":
            maxr, minr = int(f32(kpY + r)), int(f32(kpY - r))
        else:
            maxr = int(math.ceil(f32(kpY + r)))                             # :724
            minr = int(math.floor(f32(kpY - r)))                            # :725
        if minr < 0 or maxr >= nRows:
            raise SceneError(f"right key point {iR}: rows [{minr}, {maxr}] leave vRowIndices")      # :728 writes out of range
        for yi in range(minr, maxr + 1):                                    # :727
            vRowIndices[yi].append(iR)

    minZ = mb                                                               # :732
    minD = f32(0)                                                           # :733
    maxD = mbf / minZ                                                       # :734
    vDistIdx = []                                                           # :737

    for iL in range(N):                                                     # :740
        levelL = int(kpsL["octave"][iL])
        vL, uL = f32(kpsL["y"][iL]), f32(kpsL["x"][iL])
        vCandidates = vRowIndices[int(vL)]                                  # :747 (float -> size_t truncates)
        if not vCandidates:                                                 # :749
            tag[iL] = "no_row_cand"
            continue
        minU = f32(uL - maxD)                                               # :752
        maxU = f32(uL - minD)                                               # :753
        if maxU < 0:                                                        # :755
            tag[iL] = "maxU"
            continue
        bestDist, bestIdxR = TH_HIGH, 0                                     # :758-759
        dL = descL[iL]
        orange = 2 if mutate == "oct_wide" else 1
        for iR in vCandidates:                                              # :764
            octR = int(kpsR["octave"][iR])
            if octR < levelL - orange or octR > levelL + orange:            # :769
                continue
            uR = f32(kpsR["x"][iR])
            inside = (uR > minU and uR < maxU) if mutate == "u_open" else (uR >= minU and uR <= maxU)     # :774
            if inside:
                if c_round(f32(uR * f32(inv_sf[levelL]))) < 10:
                    raise SceneError(f"right key point {iR} passes the gates of left key point {iL} with scaleduR0 < 10 on level {levelL}")   # :816 could throw
                dist = hamming(dL, descR[iR])                               # :777
                if (dist <= bestDist) if mutate == "tie_last" else (dist < bestDist):                     # :779
                    bestDist, bestIdxR = dist, iR
        out_iR[iL], out_dist[iL] = bestIdxR, bestDist
        if not ((bestDist <= thOrbDist) if mutate == "th_le" else (bestDist < thOrbDist)):                # :788
            tag[iL] = "no_match"
            continue
        uR0 = f32(kpsR["x"][bestIdxR])                                      # :791
        scaleFactor = f32(inv_sf[levelL])                                   # :792
        scaleduL = rnd(f32(uL * scaleFactor))                               # :793
        scaledvL = rnd(f32(vL * scaleFactor))                               # :794
        scaleduR0 = rnd(f32(uR0 * scaleFactor))                             # :795
        w = 5                                                               # :798
        imL, imR = pyrL[levelL], pyrR[levelL]
        cy, cxL, cxR0 = int(scaledvL), int(scaleduL), int(scaleduR0)
        if cy - w < 0 or cy + w + 1 > imL.shape[0] or cxL - w < 0 or cxL + w + 1 > imL.shape[1]:
            raise SceneError(f"left key point {iL}: its 11x11 window leaves level {levelL}")              # :799 would throw
        IL = imL[cy - w:cy + w + 1, cxL - w:cxL + w + 1].astype(np.int64)   # :799-800
        IL = IL - IL[w, w]                                                  # :801
        bestDistS, bestincR = INT_MAX, 0                                    # :803-804
        L = 5                                                               # :805
        vDists = [f32(0)] * (2 * L + 1)                                     # :806-807
        iniu = f32(scaleduR0 + f32(L) - f32(w))                             # :809
        endu = f32(scaleduR0 + f32(L) + f32(w) + f32(1))                    # :810
        if mutate != "no_endu" and (iniu < 0 or endu >= imR.shape[1]):      # :811
            tag[iL] = "endu"
            continue
        if cxR0 - L - w < 0 or cxR0 + L + w + 1 > imR.shape[1]:
            raise SceneError(f"left key point {iL}: the strip around right key point {bestIdxR} leaves level {levelL}")   # :816 would throw
        for incR in range(-L, L + 1):                                       # :814
            c = cxR0 + incR
            IR = imR[cy - w:cy + w + 1, c - w:c + w + 1].astype(np.int64)   # :816-817
            IR = IR - IR[w, w]                                              # :818
            s = int(np.abs(IL - IR).sum())                                  # :820 cv::norm NORM_L1: integer-valued, exact
            if mutate == "sad15":
                s &= 0x7fff
            dist = f32(s)
            if dist < f32(bestDistS):                                       # :821 (int -> float)
                bestDistS, bestincR = int(dist), incR                       # :823-824
            vDists[L + incR] = dist                                         # :827
            out_sads[iL, L + incR] = s
        out_inc[iL] = bestincR
        if bestincR == -L or bestincR == L:                                 # :830
            if mutate != "keep_edge_inc":
                tag[iL] = "edge_inc"
                continue
        # (keep_edge_inc: the missing neighbour is read as the edge value itself)
        dist1 = vDists[max(L + bestincR - 1, 0)]                            # :834
        dist2 = vDists[L + bestincR]                                        # :835
        dist3 = vDists[min(L + bestincR + 1, 2 * L)]                        # :836
        with np.errstate(all="ignore"):
            deltaR = f32(f32(dist1 - dist3) / f32(f32(2.0) * f32(f32(dist1 + dist3) - f32(f32(2.0) * dist2))))      # :838
        if deltaR < -1 or deltaR > 1:                                       # :840
            tag[iL] = "delta"
            continue
        with np.errstate(all="ignore"):
            bestuR = f32(f32(sf[levelL]) * f32(f32(scaleduR0 + f32(bestincR)) + deltaR))                            # :844
            disparity = f32(uL - bestuR)                                    # :846
        low = (disparity > minD) if mutate == "zero_disp_reject" else (disparity >= minD)
        if low and disparity < maxD:                                        # :848
            if disparity <= 0:                                              # :850
                disparity = f32(0.01)                                       # :852
                bestuR = f32(float(uL) - 0.01)                              # :853 (double arithmetic, stored as float)
            depth[iL] = mbf / disparity                                     # :855
            uRight[iL] = bestuR                                             # :856
            vDistIdx.append((bestDistS, iL))                                # :857
            sad[iL] = bestDistS
        else:
            tag[iL] = "disparity"

    if vDistIdx:     # (an empty list reads out of range in the reference, :863; the project's convention C.5 skips the filter)
        vDistIdx.sort()                                                     # :862
        m = len(vDistIdx)
        median = f32(vDistIdx[(m - 1) // 2 if mutate == "median_lo" else m // 2][0])      # :863
        thDist = f32(f32(f32(1.5) * f32(1.4)) * median)                     # :864
        for i in range(m - 1, -1, -1):                                      # :866
            d = f32(vDistIdx[i][0])
            if (d <= thDist) if mutate == "thdist_le" else (d < thDist):    # :868
                break
            uRight[vDistIdx[i][1]] = -1                                     # :872
            depth[vDistIdx[i][1]] = -1                                      # :873
            tag[vDistIdx[i][1]] = "median"
    return dict(uRight=uRight, depth=depth, sad=sad, iR=out_iR, bestDist=out_dist, sads=out_sads, bestinc=out_inc, tag=tag)
