"""Cases for olf_search_by_bow_pairs_dev (tests/test_bow_pairs_cpu.py, tests/test_bow_pairs_gpu.py): fabricated frames, one scenario_* function per case.
Every scenario builds its case, asserts from the oracle's own output (oracle_lib.search_by_bow / search_by_bow_kf on OracleVoc.transform's feature
vectors) or from a numpy count that the case really occurs, and returns what the GPU test compares against.  Nothing here needs a device."""
import functools
import types
import numpy as np
from orb_line_slam_amd._lib import KEYPOINT_DTYPE

KF_FRAME, KF_KF = 0, 1                 # OLF_BOW_KF_FRAME, OLF_BOW_KF_KF (include/orbline.h)
TH_LOW = 50
COUNTS6 = (0, 1, 63, 64, 65, 300)
ALL_PAIRS = [(i, j) for i in range(6) for j in range(6) if i != j]
f32 = np.float32


def _flip(rng, d, bits):
    """d with exactly bits[r] distinct bits of row r flipped"""
    d = d.copy()
    for r in range(len(d)):
        for b in rng.choice(256, int(bits[r]), replace=False):
            d[r, b // 8] ^= np.uint8(1 << (b % 8))
    return d


def hamming(a, B):
    return np.unpackbits(np.bitwise_xor(a[None], B), axis=1).sum(1)


def frame(desc, angle=None, valid=None, bad=None):
    n = len(desc)
    fr = types.SimpleNamespace(desc=np.ascontiguousarray(desc, np.uint8).reshape(n, 32))
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["angle"] = np.zeros(n, f32) if angle is None else angle
    k["size"], k["class_id"] = 31, -1
    fr.keys = k
    fr.valid = np.ones(n, bool) if valid is None else valid
    fr.bad = np.zeros(n, bool) if bad is None else bad
    return fr


def make_frames(counts, seed, pool=320):
    """Frames that observe subsets of one pool of points: descriptors 0 to 12 bits from the point's; about 40 % of the features hold no point and one
    in ten of the held points is bad; angles follow the point's, three in ten are random (those matches leave the three main rotation bins)."""
    rng = np.random.default_rng(seed)
    # (the pool's descriptors form 12 clusters, 40 bits around a centre each: two views of a point then mostly descend to the same vocabulary node)
    base = _flip(rng, rng.integers(0, 256, (12, 32), dtype=np.uint8)[rng.integers(0, 12, pool)], np.full(pool, 40))
    bang = rng.uniform(0, 360, pool)
    frames = []
    for n in counts:
        obs = rng.permutation(pool if n > 70 else 70)[:n]           # (the small frames share the first 70 points)
        ang = ((bang[obs] + np.where(rng.random(n) < 0.7, rng.normal(0, 3, n), rng.uniform(0, 360, n))) % 360).astype(f32)
        ang[ang >= 360] = 0
        valid = rng.random(n) < 0.6
        fr = frame(_flip(rng, base[obs], rng.integers(0, 13, n)), ang, valid, valid & (rng.random(n) < 0.1))
        fr.obs = obs
        frames.append(fr)
    return frames, base


@functools.lru_cache(maxsize=None)
def _tree(k, L):
    import oracle_lib
    return oracle_lib.random_vocabulary(k, L, 31)


def make_voc(k, L, base, seed=5, stop_every=7):
    """centroids drawn from `base`; every stop_every-th word has weight 0 (its features are in no FeatureVector).  Returns the arrays of
    ORBVocabulary.from_arrays, the oracle's vocabulary and the leaf mask."""
    import oracle_lib
    parent, leaf, vdesc, weight = _tree(k, L)
    rng = np.random.default_rng(seed)
    vdesc = vdesc.copy()
    vdesc[1:] = base[rng.integers(0, len(base), len(parent) - 1)]
    weight = weight.copy()
    if stop_every:
        weight[np.flatnonzero(leaf)[::stop_every]] = 0.0
    return (k, L, parent, leaf, vdesc, weight), oracle_lib.OracleVoc.create(k, L, parent, leaf, vdesc, weight), np.asarray(leaf, bool)


def view(fr, V, levelsup, masks=True):
    """the frame as the oracle's searches read it; masks=False: every feature holds a good point (mp_valid = NULL, d_mp_bad = NULL)"""
    n = len(fr.keys)
    v = types.SimpleNamespace(N=n, mvKeysUn=fr.keys, mvKeys=fr.keys, mDescriptors=fr.desc)
    v.mp_valid = fr.valid if masks else np.ones(n, bool)
    v.mp_bad = fr.bad if masks else np.zeros(n, bool)
    v.mFeatVec = V.transform(fr.desc, levelsup)[1] if n else {}
    return v


def oracle_pairs(views, pairs, form, nnratio, check):
    """[(nmatches, row)] per pair: the row is indexed by the feature of F (KF_FRAME) or by idx1 (KF_KF)"""
    import oracle_lib
    fn = oracle_lib.search_by_bow if form == KF_FRAME else oracle_lib.search_by_bow_kf
    out = []
    for a, b in pairs:
        n, row = fn(views[a], views[b], nnratio, checkOri=check)
        out.append((int(n), np.array(row, np.int32)))
    return out


def walk(v1, v2, form, nnratio):
    """numpy mirror of the two overloads without the rotation check, for counting cases only.  Returns (row, events): one event per searched feature of
    the first frame with a free candidate -- i1, b1, b2, the free candidates at the minimum distance as places in the node's segment of the second
    frame (`ties`), the place of the first other candidate at the second-best distance (`second`, None: none), the segment's length and `accepted`."""
    row = np.full(v2.N if form == KF_FRAME else v1.N, -1, np.int32)
    taken = np.zeros(v2.N, bool) if form == KF_FRAME else ~(v2.mp_valid & ~v2.mp_bad)
    events = []
    for node in sorted(v1.mFeatVec):
        if node not in v2.mFeatVec:
            continue
        c = np.asarray(v2.mFeatVec[node])
        for i1 in v1.mFeatVec[node]:
            if not v1.mp_valid[i1] or v1.mp_bad[i1]:
                continue
            free = np.flatnonzero(~taken[c])
            if not len(free):
                continue
            d = hamming(v1.mDescriptors[i1], v2.mDescriptors[c[free]])
            order = np.lexsort((free, d))
            b1, best = int(d[order[0]]), int(free[order[0]])
            b2, second = (int(d[order[1]]), int(free[order[1]])) if len(free) > 1 else (256, None)
            ok = (b1 <= TH_LOW if form == KF_FRAME else b1 < TH_LOW) and f32(b1) < f32(nnratio) * f32(b2)
            events.append(types.SimpleNamespace(i1=i1, b1=b1, b2=b2, best=best, second=second, ties=[int(p) for p in free[d == b1]], seg=len(c), accepted=bool(ok)))
            if ok:
                taken[c[best]] = True
                if form == KF_FRAME:
                    row[c[best]] = i1
                else:
                    row[i1] = c[best]
    return row, events


# ---- scenarios ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames6():
    return make_frames(COUNTS6, 17)


# (k, L, levelsup): the node level is the root (one serial chain, segments over 64), the leaves, and one level between
TREES = [(4, 2, 2), (4, 3, 0), (4, 3, 1)]


@functools.lru_cache(maxsize=None)
def scenario_all_pairs(k, L, levelsup, form, check, masks=True):
    frames, base = frames6()
    voc, V, leaf = make_voc(k, L, base)
    views = [view(fr, V, levelsup, masks) for fr in frames]
    nodes = set().union(*[set(v.mFeatVec) for v in views])
    if levelsup >= L:
        assert nodes == {0} and len(views[5].mFeatVec[0]) > 3 * 64                     # the root: one chain, four chunks and more
    elif levelsup == 0:
        assert len(nodes) > 4 and all(leaf[n] for n in nodes)                           # the leaves
    else:
        assert len(nodes) > 1 and not any(leaf[n] for n in nodes) and 0 not in nodes
    assert sum(len(l) for l in views[5].mFeatVec.values()) < views[5].N                 # words of weight 0: features in no FeatureVector
    if masks:
        assert all(0.25 < 1 - fr.valid.mean() < 0.55 for fr in frames[2:]) and sum(int(fr.bad.sum()) for fr in frames) > 10
    exp = oracle_pairs(views, ALL_PAIRS, form, 0.7, check)
    total = sum(n for n, _ in exp)
    assert total > 50
    if check:
        free = oracle_pairs(views, ALL_PAIRS, form, 0.7, False)
        assert sum(n for n, _ in free) > total                                          # the histogram drops matches somewhere
    for (a, b), (n, row) in zip(ALL_PAIRS, exp):
        assert len(row) == (views[b].N if form == KF_FRAME else views[a].N) and n == (row >= 0).sum()
    return frames, voc, exp


@functools.lru_cache(maxsize=None)
def scenario_ties():
    """One node (the root) holds every feature.  Forty features of the second frame exist twice: thirty 70 places apart (the two copies sit in different
    chunks of 64), ten next to each other (the same chunk).  With nnratio 1.2 an equal best and second best passes the ratio test and the winner shows; with 0.9
    it fails.  Returns the expectations of [(0, 1), (1, 0)] in both forms under both ratios."""
    frames, base = make_frames((200, 200), 23, pool=260)
    f1, f2 = frames
    where1 = {int(p): i for i, p in enumerate(f1.obs)}
    across = [(t, t + 70) for t in range(60) if int(f2.obs[t]) in where1][:30]          # places 0 .. 59 and 70 .. 129: chunk 0 and chunk 1 or 2
    inside = [(t, t + 1) for t in range(132, 190, 3) if int(f2.obs[t]) in where1 and t % 64 < 63][:10]
    assert len(across) == 30 and len(inside) == 10
    for a, b in across + inside:
        i1 = where1[int(f2.obs[a])]
        f1.valid[i1], f1.bad[i1] = True, False
        f2.desc[b], f2.keys[b] = f2.desc[a], f2.keys[a]
        f2.valid[a] = f2.valid[b] = True
        f2.bad[a] = f2.bad[b] = False
    voc, V, _ = make_voc(4, 2, base, stop_every=0)
    views = [view(fr, V, 2) for fr in frames]
    assert list(views[1].mFeatVec) == [0] and len(views[1].mFeatVec[0]) == 200          # a segment of the second frame longer than 64: four chunks
    pairs = [(0, 1), (1, 0)]
    exp = {}
    for form in (KF_FRAME, KF_KF):
        for ratio in (1.2, 0.9):
            exp[form, ratio] = oracle_pairs(views, pairs, form, ratio, True)
            row, ev = walk(views[0], views[1], form, ratio)
            assert np.array_equal(row, oracle_pairs(views, [(0, 1)], form, ratio, False)[0][1])      # the mirror is the oracle
            chunk = lambda p: p // 64
            tied = [e for e in ev if len(e.ties) > 1]
            across = [e for e in tied if chunk(e.ties[0]) != chunk(e.ties[1])]
            assert len(across) >= 5 and len(tied) - len(across) >= 3                    # equal minima on both sides of a chunk boundary, and inside a chunk
            assert all(e.best == e.ties[0] for e in tied)                               # the earlier one is the best
            assert all(e.b1 == e.b2 for e in tied)
            if ratio > 1:
                won = [e for e in across if e.accepted]
                assert len(won) >= 5
                c = views[1].mFeatVec[0]
                for e in won:                                                           # ... and the oracle's row names it, not the later copy
                    assert (row[c[e.best]] == e.i1) if form == KF_FRAME else (row[e.i1] == c[e.best])
            else:
                assert not any(e.accepted for e in tied)                                # bestDist1 == bestDist2: the ratio test fails
                assert sum(1 for e in tied if e.b1 < TH_LOW) >= 5
            assert sum(1 for e in ev if e.accepted and chunk(e.best) >= 1) >= 5         # a best candidate in the second chunk or later
            two = [e for e in ev if e.second is not None]
            assert sum(1 for e in two if chunk(e.best) == chunk(e.second)) >= 5 and sum(1 for e in two if chunk(e.best) != chunk(e.second)) >= 5
    return frames, voc, pairs, exp


def _rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def scenario_thresholds():
    """The root holds everything.  Feature 0 of frame 0 has its nearest candidate at exactly TH_LOW = 50 bits and nothing else near: the frame form
    accepts it (<=), the key-frame form does not (<).  Feature 1 has candidates at 30 and 40 bits: 30 < 0.75 * 40 is false, the ratio test fails
    at equality.  Feature 2 is the control, 10 bits from its candidate: both forms accept it."""
    rng = np.random.default_rng(41)
    A = _rand_desc(rng, 3)
    B = np.concatenate([_flip(rng, A[[0, 1, 1, 2]], [50, 30, 40, 10]), _rand_desc(rng, 70)])
    frames = [frame(A), frame(B)]
    voc, V, _ = make_voc(4, 2, np.concatenate([A, B]), stop_every=0)
    views = [view(fr, V, 2) for fr in frames]
    assert list(views[0].mFeatVec) == [0] and list(views[1].mFeatVec) == [0]
    exp = {form: oracle_pairs(views, [(0, 1)], form, 0.75, True) for form in (KF_FRAME, KF_KF)}
    for form in exp:
        _, ev = walk(views[0], views[1], form, 0.75)
        e = {x.i1: x for x in ev}
        assert (e[0].b1, e[0].best) == (50, 0) and e[0].b2 > 90 and (e[1].b1, e[1].b2) == (30, 40) and e[2].b1 == 10
    (nf, rowf), (nk, rowk) = exp[KF_FRAME][0], exp[KF_KF][0]
    assert nf == 2 and rowf[0] == 0 and rowf[3] == 2 and (rowf[[1, 2]] == -1).all()      # the frame form accepts the distance of 50 ...
    assert nk == 1 and rowk[0] == -1 and rowk[1] == -1 and rowk[2] == 3                  # ... the key-frame form rejects it; 30 / 40 fails in both
    return frames, voc, [(0, 1)], exp


@functools.lru_cache(maxsize=None)
def scenario_greedy():
    """Two features of the first frame in one node whose nearest candidate is the same feature of the second frame, twice: features 0 and 1 (1 then
    takes its next candidate, 20 bits away), features 2 and 3 (3 has no other candidate within TH_LOW and ends with nothing)."""
    rng = np.random.default_rng(43)
    a = _rand_desc(rng, 2)
    A = np.stack([a[0], _flip(rng, a[:1], [2])[0], a[1], _flip(rng, a[1:], [2])[0]])
    B = np.concatenate([_flip(rng, A[[0, 1, 2]], [1, 20, 1]), _rand_desc(rng, 70)])
    frames = [frame(A), frame(B)]
    voc, V, _ = make_voc(4, 2, np.concatenate([A, B]), stop_every=0)
    views = [view(fr, V, 2) for fr in frames]
    assert list(views[0].mFeatVec) == [0] and list(views[1].mFeatVec) == [0]
    for q, near in ((0, 0), (1, 0), (2, 2), (3, 2)):                                    # were the second frame untouched, both of a couple would take the same feature
        assert int(np.argmin(hamming(A[q], B))) == near
    exp = {form: oracle_pairs(views, [(0, 1)], form, 0.75, False) for form in (KF_FRAME, KF_KF)}
    (nf, rowf), (nk, rowk) = exp[KF_FRAME][0], exp[KF_KF][0]
    assert nf == 3 and list(rowf[:3]) == [0, 1, 2] and (rowf[3:] == -1).all()            # B0 <- A0, B1 <- A1 (its next candidate), B2 <- A2, A3: nothing
    assert nk == 3 and list(rowk) == [0, 1, 2, -1]
    return frames, voc, [(0, 1)], exp


@functools.lru_cache(maxsize=None)
def scenario_rotation():
    """per form and pair: matches outside the three kept bins are dropped, and the count goes down with them"""
    frames, base = frames6()
    voc, V, _ = make_voc(4, 3, base)
    views = [view(fr, V, 1) for fr in frames]
    pairs = [(5, 4), (4, 5), (5, 3)]
    exp = {}
    for form in (KF_FRAME, KF_KF):
        exp[form] = oracle_pairs(views, pairs, form, 0.7, True)
        free = oracle_pairs(views, pairs, form, 0.7, False)
        for (n, row), (n0, row0) in zip(exp[form], free):
            assert n < n0 and (row >= 0).sum() == n and ((row0 >= 0) & (row < 0)).sum() == n0 - n
    return frames, voc, pairs, exp


EDGE_GOOD = [(5, 3), (3, 5), (5, 3), (5, 4), (5, 2), (5, 1), (5, 0), (0, 5), (4, 5), (2, 4)]      # a duplicate, both orders, frame 5 in eight pairs
EDGE_BAD = [(-1, 2), (6, 1), (3, 3), (2, 6), (4, -1)]


@functools.lru_cache(maxsize=None)
def scenario_edges(form):
    """the call's pair list: EDGE_GOOD with the refused pairs of EDGE_BAD set between them"""
    frames, base = frames6()
    voc, V, _ = make_voc(4, 3, base)
    views = [view(fr, V, 1) for fr in frames]
    pairs = EDGE_GOOD[:3] + EDGE_BAD[:2] + EDGE_GOOD[3:6] + EDGE_BAD[2:3] + EDGE_GOOD[6:] + EDGE_BAD[3:]
    good_at = [q for q, p in enumerate(pairs) if p not in EDGE_BAD]
    bad_at = [q for q, p in enumerate(pairs) if p in EDGE_BAD]
    assert len(bad_at) == 5 and [pairs[q] for q in good_at] == EDGE_GOOD
    exp = oracle_pairs(views, EDGE_GOOD, form, 0.7, True)
    assert sum(n for n, _ in exp) > 20 and np.array_equal(exp[0][1], exp[2][1])
    return frames, voc, pairs, good_at, bad_at, exp


@functools.lru_cache(maxsize=None)
def scenario_consecutive():
    frames, base = frames6()
    frames = [frames[i] for i in (5, 4, 3, 5, 2, 1, 0, 4)]
    voc, V, _ = make_voc(4, 3, base)
    views = [view(fr, V, 1) for fr in frames]
    pairs = [(j, j + 1) for j in range(len(frames) - 1)]
    exp = oracle_pairs(views, pairs, KF_FRAME, 0.7, True)
    assert sum(n for n, _ in exp) > 20
    return frames, voc, pairs, exp


ALL_SCENARIOS = ([(scenario_all_pairs, t + (form, check)) for t in TREES for form in (KF_FRAME, KF_KF) for check in (False, True)] +
                 [(scenario_all_pairs, (4, 3, 1, form, True, False)) for form in (KF_FRAME, KF_KF)] +
                 [(scenario_ties, ()), (scenario_thresholds, ()), (scenario_greedy, ()), (scenario_rotation, ()), (scenario_edges, (KF_FRAME,)),
                  (scenario_edges, (KF_KF,)), (scenario_consecutive, ())])
