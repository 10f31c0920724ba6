"""Scenes of the key-frame database tests.  A scene is a list of operations (add, erase, a batch of queries of one form); run_reference() plays it on the
restatement (kfdb_reference.py), run_library() on the library, either through olf_kfdb_select fed the restatement's tables (no device) or through
olf_kfdb_detect.  Key frames are named; both runners report candidates as slots (the order of the add operations) and the final per-slot state.
Every scenario function builds its scene and asserts, from the restatement alone, that the case it is named after occurs.

A key frame that is erased and added again is a new key frame object in both runners: the library gives it a new slot, whose state starts at 0.
"""
import numpy as np
import kfdb_reference as R

LOOP, LOOP_LINE, RELOC, RELOC_LINE = range(4)


def u(words, scale=1.0):
    """a BoW vector with the same weight on every word, L1 norm `scale`"""
    words = list(words)
    return {int(w): scale / len(words) for w in words}


class Scene:
    def __init__(self, n_words_p=64, n_words_l=32):
        self.n_words_p, self.n_words_l, self.ops, self.covis = n_words_p, n_words_l, [], {}

    def add(self, name, bow, bow_l=(), covis=()):
        self.ops.append(("add", name, dict(bow), dict(bow_l)))
        self.covis[name] = list(covis)
        return self

    def erase(self, name):
        self.ops.append(("erase", name))
        return self

    def query(self, form, queries, minScore=0.0, invalid=False):
        """queries: dicts with mnId, bow and optionally bow_l, N, N_l, connected (names)"""
        self.ops.append(("query", form, [dict(q) for q in queries], minScore, invalid))
        return self


def run_reference(scene, want_tables=False):
    """-> (per query operation the candidate slots of each query, final state per slot[, the tables of each query operation])"""
    db = R.KeyFrameDatabase(R.Vocabulary(scene.n_words_p), R.Vocabulary(scene.n_words_l))
    named, outside, slot_kf, live, results, tabs = {}, {}, [], [], [], []
    slot_of = {}
    for op in scene.ops:
        if op[0] == "add":
            kf = R.KeyFrame(len(slot_kf), op[2], op[3] if scene.n_words_l else (), name=op[1])
            named[op[1]] = kf
            slot_of[kf] = len(slot_kf)
            slot_kf.append(kf); live.append(True)
            db.add(kf)
        elif op[0] == "erase":
            db.erase(named[op[1]])
            live[slot_of[named[op[1]]]] = False
        else:
            _, form, queries, minScore, invalid = op
            if invalid:
                results.append(None); tabs.append(None)
                continue
            for name, kf in named.items():              # the covisibility graph as it stands now; a name that was never added is a key frame outside the database
                kf.best_covisibles = [named[n] if n in named else outside.setdefault(n, R.KeyFrame(-1, {}, name=n)) for n in scene.covis[name]]
            ms = np.broadcast_to(np.asarray(minScore, np.float32), (len(queries),))
            out, qk = [], []
            for i, q in enumerate(queries):
                f = R.KeyFrame(q["mnId"], q["bow"], q.get("bow_l", ()), q.get("N", 0), q.get("N_l", 0))
                f.connected = {named[n] for n in q.get("connected", ()) if n in named}
                qk.append(f)
                fn = (db.DetectLoopCandidates, db.DetectLoopCandidatesWithLine, db.DetectRelocalizationCandidates, db.DetectRelocalizationCandidatesWithLine)[form]
                res = fn(f, ms[i]) if form in (LOOP, LOOP_LINE) else fn(f)
                out.append([slot_of[k] for k in res])
            results.append(out)
            if want_tables:
                vp = [kf.mBowVec if live[k] else [] for k, kf in enumerate(slot_kf)]
                vl = [kf.mBowVec_l if live[k] else [] for k, kf in enumerate(slot_kf)]
                tabs.append((R.tables([f.mBowVec for f in qk], vp), R.tables([f.mBowVec_l for f in qk], vl)))
    state = {k: np.array([getattr(kf, k) for kf in slot_kf], np.float32) for k in ("mRelocScore", "mRelocScore_l", "mRelocScore_pl")}
    return (results, state, tabs) if want_tables else (results, state)


def run_library(scene, mode, context=None, tables=None):
    """mode "select": olf_kfdb_select with `tables` (run_reference's); mode "detect": olf_kfdb_detect on `context`"""
    from orb_line_slam_amd import _lib
    from orb_line_slam_amd.database import KeyFrameDatabase, Query
    db = KeyFrameDatabase(scene.n_words_p, scene.n_words_l, context=context if mode == "detect" else None)
    named, results, n_query = {}, [], 0
    for op in scene.ops:
        if op[0] == "add":
            named[op[1]] = db.add(op[2], op[3])
        elif op[0] == "erase":
            db.erase(named[op[1]])
        else:
            _, form, queries, minScore, invalid = op
            qs = [Query(q["mnId"], q["bow"], q.get("bow_l"), q.get("N", 0), q.get("N_l", 0), tuple(named[n] for n in q.get("connected", ()) if n in named))
                  for q in queries]
            nb = {slot: [named.get(n, -1) for n in scene.covis[name]] for name, slot in named.items()}
            try:
                if mode == "detect":
                    out = db.detect(form, qs, minScore, nb)
                else:
                    n = db.size()[0]
                    if tables is not None and tables[n_query] is not None:
                        tp, tl = tables[n_query]
                    else:       # an operation the restatement does not play (it is refused): any tables of the right shape
                        tp = tl = {"common": np.zeros((len(qs), n), np.int32), "first": np.full((len(qs), n), -1, np.int32), "score": np.zeros((len(qs), n))}
                    out = db.select(form, qs, tp, tl, minScore, nb)
                assert not invalid, "a query operation that must be refused was accepted"
                results.append(out)
            except _lib.OlfError as e:
                assert invalid and e.code == _lib.OLF_ERR_INVALID, str(e)
                results.append(None)
            n_query += 1
    state = db.state()
    db.close()
    return results, state


def same_state(a, b):
    return all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
def empty_query():
    s = Scene().add("A", u(range(0, 10)), u(range(0, 4))).query(RELOC, [dict(mnId=1, bow={})]).query(RELOC_LINE, [dict(mnId=2, bow={}, bow_l={}, N=5, N_l=5)])
    res, _ = run_reference(s)
    assert res == [[[]], [[]]]
    return s


def no_shared_word():
    s = Scene().add("A", u(range(0, 10))).add("B", u(range(10, 20))).query(RELOC, [dict(mnId=1, bow=u(range(30, 40)))])
    s.query(LOOP, [dict(mnId=1, bow=u(range(30, 40)))], 0.0)
    res, _ = run_reference(s)
    assert res == [[[]], [[]]]
    return s


def _stale_scene(batch):
    A, B, C = u(list(range(0, 5)) + list(range(40, 55))), u([0] + list(range(30, 39))), u(list(range(4, 10)) + list(range(56, 60)))
    s = Scene().add("A", A, covis=["B"]).add("B", B).add("C", C)
    q1, q2 = dict(mnId=1, bow=B), dict(mnId=2, bow=u(range(0, 10)))
    return s.query(RELOC, [q1, q2] if batch else [q2])


def stale_reloc_score():
    """query 1 scores B (1.0).  Query 2 shares one word with B, too few to score it, but scores A whose neighbour B is: the gate :476 lets B's old score
    into A's sum, which makes B the candidate in place of C"""
    s = _stale_scene(True)
    (both,), state = run_reference(s)
    (alone,), _ = run_reference(_stale_scene(False))
    assert both[1] == [1] and alone[0] == [2], (both, alone)
    assert state["mRelocScore"][1] == np.float32(1.0)
    return s


def _connected_scene(connected):
    # A is the query itself (score 1); B has 9 of its 10 words among 20 of its own (score 0.45): scored, but below 0.75 of A's
    s = Scene().add("A", u(range(0, 10))).add("B", u(list(range(0, 9)) + list(range(20, 31))))
    return s.query(LOOP, [dict(mnId=1, bow=u(range(0, 10)), connected=["A"] if connected else [])], 0.1)


def connected_would_have_won():
    (free,), _ = run_reference(_connected_scene(False))
    s = _connected_scene(True)
    (held,), _ = run_reference(s)
    assert free[0] == [0] and held[0] == [1], (free, held)
    return s


def _best_scene(covis_x, covis_y):
    # X: 5 of the query's 10 words, Y: 6 of them; both are scored (minCommonWords = 4)
    X, Y = u(list(range(0, 5)) + list(range(20, 25))), u(list(range(4, 10)) + list(range(30, 34)))
    return Scene().add("X", X, covis=covis_x).add("Y", Y, covis=covis_y).query(RELOC, [dict(mnId=1, bow=u(range(0, 10)))])


def pbest_differs():
    """X's neighbour Y scores higher: X's entry names Y (sum 1.1); Y's own entry (0.6) falls below 0.75 * 1.1"""
    (plain,), _ = run_reference(_best_scene([], []))
    s = _best_scene(["Y"], [])
    (res,), _ = run_reference(s)
    assert plain[0] == [0, 1] and res[0] == [1], (plain, res)
    return s


def duplicate_best_removed():
    """both entries name Y with the same sum: the second is a duplicate"""
    s = _best_scene(["Y"], ["X"])
    seen, orig = [], R.KeyFrameDatabase._retain
    R.KeyFrameDatabase._retain = staticmethod(lambda acc, best: (seen.append((list(acc), best)), orig(acc, best))[1])
    try:
        (res,), _ = run_reference(s)
    finally:
        R.KeyFrameDatabase._retain = staticmethod(orig)
    (acc, best), = seen
    assert res[0] == [1] and len(acc) == 2 and acc[0][1] is acc[1][1] and all(a > np.float32(0.75) * best for a, _ in acc)
    return s


def score_equal_to_minscore():
    """si == minScore: kept by >= in the plain loop form (:167), dropped by > in the WithLine form (:339); N_l = 0 makes score_pl = spi * N / N = spi"""
    A, q = u(list(range(0, 6)) + [20, 21]), u(range(0, 8))
    si = np.float32(R.l1_score(sorted(q.items()), sorted(A.items())))
    s = Scene().add("A", A, u([1]))
    s.query(LOOP, [dict(mnId=1, bow=q)], si).query(LOOP_LINE, [dict(mnId=2, bow=q, bow_l=u([1]), N=3, N_l=0)], si)
    res, _ = run_reference(s)
    assert np.float32(si * np.float32(3)) / np.float32(3) == si
    assert res == [[[0]], [[]]], res
    return s


def union_through_lines_only():
    """L shares no point word with the query: it enters sKFsSharingWords_pl through lKFsSharingWords_l alone, and its point score is -0.0"""
    s = Scene().add("P", u(range(0, 10)), u(range(0, 4))).add("L", u(range(40, 50)), u(range(8, 12)))
    s.query(RELOC_LINE, [dict(mnId=1, bow=u(range(0, 10)), bow_l=u(range(8, 12)), N=10, N_l=10)])
    (res,), state, tabs = run_reference(s, want_tables=True)
    assert tabs[0][0]["common"][0, 1] == 0 and tabs[0][1]["common"][0, 1] == 4
    assert res[0] == [0, 1] and state["mRelocScore_l"][1] == 1 and np.signbit(state["mRelocScore"][1]) and state["mRelocScore_pl"][1] == 0.5
    return s


def erase_then_add_changes_order():
    """A and B share the query's first word; A was added first.  Erased and added again, A stands behind B in every posting list"""
    A, B, q = u(range(0, 10)), u(range(0, 10)), u(range(0, 10))
    s = Scene().add("A", A).add("B", B).query(RELOC, [dict(mnId=1, bow=q)]).erase("A").add("A", A).query(RELOC, [dict(mnId=2, bow=q)])
    res, _ = run_reference(s)
    assert res == [[[0, 1]], [[1, 2]]], res
    return s


def no_features_at_all():
    """np + nl == 0: score_pl is 0 / 0 = NaN, no comparison with it holds, nothing is retained -- and the NaN stays in mRelocScore_pl"""
    s = Scene().add("A", u(range(0, 10)), u(range(0, 4))).query(RELOC_LINE, [dict(mnId=1, bow=u(range(0, 10)), bow_l=u(range(0, 4)), N=0, N_l=0)])
    s.query(LOOP_LINE, [dict(mnId=1, bow=u(range(0, 10)), bow_l=u(range(0, 4)), N=0, N_l=0)], 0.0)
    res, state = run_reference(s)
    assert res == [[[]], [[]]] and np.isnan(state["mRelocScore_pl"][0]) and state["mRelocScore"][0] == 1
    return s


def neighbour_outside_database():
    s = _best_scene(["never added", "Y"], [])
    (res,), _ = run_reference(s)
    assert res[0] == [1] and "never added" not in [op[1] for op in s.ops if op[0] == "add"]
    return s


def non_increasing_id_refused():
    q = u(range(0, 10))
    s = Scene().add("A", q).query(RELOC, [dict(mnId=5, bow=q)]).query(RELOC, [dict(mnId=5, bow=q)], invalid=True)
    s.query(RELOC_LINE, [dict(mnId=4, bow=q, N=1, N_l=1)], invalid=True).query(RELOC, [dict(mnId=6, bow=q), dict(mnId=6, bow=q)], invalid=True)
    s.query(LOOP, [dict(mnId=0, bow=q)], 0.0, invalid=True).query(LOOP, [dict(mnId=1, bow=q)], 0.0)      # the loop family has its own counter; 0 is the constructor's value
    res, _ = run_reference(s)
    assert res[0] == [[0]] and res[-1] == [[0]] and res[1:5] == [None] * 4
    return s


ALL_SCENARIOS = [empty_query, no_shared_word, stale_reloc_score, connected_would_have_won, pbest_differs, duplicate_best_removed, score_equal_to_minscore,
                 union_through_lines_only, erase_then_add_changes_order, no_features_at_all, neighbour_outside_database, non_increasing_id_refused]


def random_scene(seed, n_kf=40, n_queries=17):
    """a database of random key frames with a random covisibility graph and, per family, a batch of n_queries mixed queries in the plain and in the
    WithLine form: empty ones, copies of key frames, random ones, some connected to key frames"""
    rng = np.random.default_rng(seed)
    s = Scene(200, 60)

    def vec(n_words, lo, hi):
        w = np.sort(rng.choice(n_words, int(rng.integers(lo, hi)), replace=False))
        v = rng.random(len(w)) + 0.05
        return dict(zip(w.tolist(), (v / v.sum()).tolist()))

    names = [f"kf{i}" for i in range(n_kf)]
    bows = {}
    for i, n in enumerate(names):
        bows[n] = (vec(200, 10, 40), vec(60, 3, 15))
        nb = [names[j] for j in rng.choice(n_kf, int(rng.integers(0, 11)), replace=False) if j != i]
        s.add(n, *bows[n], covis=nb + (["outside"] if i % 7 == 0 else []))
    s.erase(names[5])
    next_id = {LOOP: 1, RELOC: 1}
    for form in (RELOC, LOOP, RELOC_LINE, LOOP_LINE, RELOC):
        fam = LOOP if form in (LOOP, LOOP_LINE) else RELOC
        qs = []
        for i in range(n_queries):
            kind = i % 4
            bp, bl = ({}, {}) if kind == 0 and i < 4 else bows[names[int(rng.integers(n_kf))]] if kind == 1 else (vec(200, 10, 40), vec(60, 3, 15))
            qs.append(dict(mnId=next_id[fam], bow=bp, bow_l=bl, N=int(rng.integers(0, 1000)), N_l=int(rng.integers(0, 200)),
                           connected=[names[j] for j in rng.choice(n_kf, int(rng.integers(0, 6)), replace=False)]))
            next_id[fam] += int(rng.integers(1, 4))
        s.query(form, qs, rng.uniform(0.0, 0.05, n_queries).astype(np.float32))
    return s
