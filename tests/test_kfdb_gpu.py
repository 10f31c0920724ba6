"""The key-frame database on the device: olf_kfdb_tables_dev, olf_kfdb_detect, olf_bow_score_pairs_dev and olf_bow_score against the restatement
(kfdb_reference.py).  BoW vectors are made directly from seeded random word ids and L1-normalised weights: no vocabulary tree is needed.  Scores are compared
as 64-bit patterns."""
import ctypes as C
import os
import subprocess
import numpy as np
import pytest
import kfdb_reference as R
import kfdb_scenes as S
from orb_line_slam_amd import _lib
from orb_line_slam_amd._lib import OLF_ERR_CAPACITY, OLF_ERR_INVALID, last_error, lib
from orb_line_slam_amd.database import KeyFrameDatabase, Query
from orb_line_slam_amd.vocabulary import ORBVocabulary

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = (0, 1, 63, 64, 65, 257, 2000)       # words per vector: around the 64 lanes of a wave, several chunks, and more than the word ids of the small space
N_IDS, N_IDS_WIDE = 1000, 2500              # a BowVector's ids are distinct, so a 2000-word vector cannot come from 1000 ids: those draw from 2500 (and still
                                            # share hundreds of words with every other vector); every other vector draws from the first 1000


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(_lib.default_params(), 640, 480, 1)
    yield c
    c.close()


def vector(rng, n, n_ids=None):
    n_ids = n_ids or (N_IDS_WIDE if n > N_IDS else N_IDS)
    ids = np.sort(rng.choice(n_ids, n, replace=False)).astype(np.int32)
    w = rng.random(n) + 1e-3
    return ids, w / w.sum() if n else w


def as_list(v):
    return list(zip(v[0].tolist(), v[1].tolist()))


def same_tables(got, want):
    assert np.array_equal(got["common"], want["common"])
    assert np.array_equal(got["first"], want["first"])
    assert np.array_equal(got["score"].view(np.uint64), want["score"].view(np.uint64))


def build(ctx, rng, n_slots, n_ids=N_IDS_WIDE, sizes=SIZES):
    """a database of n_slots vectors whose sizes cycle through `sizes` (starting somewhere else for every size of database), the middle one erased"""
    db = KeyFrameDatabase(n_ids, context=ctx)
    kfs = [vector(rng, sizes[(k + n_slots) % len(sizes)], None if n_ids == N_IDS_WIDE else n_ids) for k in range(n_slots)]
    for v in kfs:
        db.add(v)
    slots = [as_list(v) for v in kfs]
    if n_slots >= 3:
        db.erase(n_slots // 2)
        slots[n_slots // 2] = []
    return db, kfs, slots


@pytest.mark.parametrize("n_queries", [1, 3, 17])
@pytest.mark.parametrize("n_slots", [1, 2, 63, 64, 65, 300])
def test_tables_equal_restatement(ctx, n_slots, n_queries):
    rng = np.random.default_rng(1000 * n_slots + n_queries)
    db, kfs, slots = build(ctx, rng, n_slots)
    twin = max((k for k in range(n_slots) if slots[k]), key=lambda k: len(slots[k]), default=None)      # a live key frame with words, the longest
    queries = [kfs[twin]] if twin is not None else [vector(rng, 64)]                                   # one query identical to a key frame
    queries += [vector(rng, 0)]                                                                         # one empty query
    queries += [vector(rng, SIZES[(i + 2) % len(SIZES)]) for i in range(n_queries)]
    batches = [queries[:1], queries[1:2]] if n_queries == 1 else [queries[:n_queries]]
    for batch in batches:
        got = db.tables(batch)
        want = R.tables([as_list(q) for q in batch], slots)
        same_tables(got, want)
        assert got["common"].shape == (len(batch), n_slots)
        if batch[0] is queries[0] and twin is not None:
            assert got["common"][0, twin] == len(slots[twin]) and np.float32(got["score"][0, twin]) == np.float32(1.0)
        if n_slots >= 3:
            e = n_slots // 2
            assert (got["common"][:, e] == 0).all() and (got["first"][:, e] == -1).all() and (got["score"][:, e].view(np.uint64) == 0x8000000000000000).all()
        for i, q in enumerate(batch):
            if len(q[0]) == 0:
                assert (got["common"][i] == 0).all() and (got["score"][i].view(np.uint64) == 0x8000000000000000).all()
    db.close()


def test_tables_with_both_vocabularies(ctx):
    """the point and the line tables of one call, from different queries against different vectors"""
    rng = np.random.default_rng(5)
    db = KeyFrameDatabase(1000, 200, context=ctx)
    kp, kl = [vector(rng, n) for n in (65, 0, 257, 64)], [vector(rng, n, 200) for n in (30, 64, 0, 65)]
    for a, b in zip(kp, kl):
        db.add(a, b)
    qp, ql = [vector(rng, n) for n in (64, 0, 300)], [vector(rng, n, 200) for n in (0, 65, 100)]
    gp, gl = db.tables(qp, ql)
    same_tables(gp, R.tables([as_list(q) for q in qp], [as_list(v) for v in kp]))
    same_tables(gl, R.tables([as_list(q) for q in ql], [as_list(v) for v in kl]))
    db.close()


def test_tables_over_a_million_word_ids(ctx):
    """the realistic regime: 10^6 word ids, 1000-word vectors, about one common word per pair -- and many pairs with none"""
    rng = np.random.default_rng(11)
    db, kfs, slots = build(ctx, rng, 65, n_ids=10**6, sizes=(1000, 990, 1010))
    queries = [vector(rng, 1000, 10**6), kfs[7], vector(rng, 0), vector(rng, 1010, 10**6)]         # random, a key frame's twin, empty, random
    got = db.tables(queries)
    want = R.tables([as_list(q) for q in queries], slots)
    others = np.delete(want["common"][[0, 3]], 7, axis=1)
    assert 0.5 < others.mean() < 2.0 and (others == 0).any() and (others > 1).any()
    same_tables(got, want)
    assert got["common"][1, 7] == len(slots[7]) and np.float32(got["score"][1, 7]) == np.float32(1.0) and (got["common"][:, 32] == 0).all()
    db.close()


def test_score_is_the_sum_in_ascending_word_order(ctx):
    """The restatement first shows that the order matters: the same terms summed in reverse order, and summed pairwise (a tree), change the bits of at least
    one score.  The device must equal the in-order sum everywhere, which a tree or butterfly reduction of the terms cannot."""
    rng = np.random.default_rng(3)

    def wide(n):
        ids = np.sort(rng.choice(300, n, replace=False)).astype(np.int32)
        w = np.exp(rng.normal(0, 3, n))
        return ids, w / w.sum()

    kfs, queries = [wide(257) for _ in range(8)], [wide(257) for _ in range(3)]

    def terms(v1, v2):
        a, b = dict(as_list(v1)), dict(as_list(v2))
        return [abs(a[w] - b[w]) - abs(a[w]) - abs(b[w]) for w in sorted(set(a) & set(b))]

    def in_order(t):
        s = 0.0
        for x in t:
            s += x
        return -s / 2.0

    def pairwise(t):
        t = list(t)
        while len(t) > 1:
            t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
        return -t[0] / 2.0

    fwd = np.array([[in_order(terms(q, k)) for k in kfs] for q in queries])
    rev = np.array([[in_order(terms(q, k)[::-1]) for k in kfs] for q in queries])
    tree = np.array([[pairwise(terms(q, k)) for k in kfs] for q in queries])
    want = R.tables([as_list(q) for q in queries], [as_list(k) for k in kfs])
    assert np.array_equal(fwd.view(np.uint64), want["score"].view(np.uint64))
    assert (fwd.view(np.uint64) != rev.view(np.uint64)).any() and (fwd.view(np.uint64) != tree.view(np.uint64)).any()
    db = KeyFrameDatabase(300, context=ctx)
    for k in kfs:
        db.add(k)
    same_tables(db.tables(queries), want)
    db.close()


# ---- detect -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", S.ALL_SCENARIOS, ids=lambda f: f.__name__)
def test_detect_equals_restatement(ctx, scenario):
    scene = scenario()
    want, want_state = S.run_reference(scene)
    got, got_state = S.run_library(scene, "detect", context=ctx)
    assert got == want
    assert S.same_state(got_state, want_state)


@pytest.mark.parametrize("seed", [1, 2])
def test_detect_equals_restatement_on_batches_of_17(ctx, seed):
    """per family a batch of 17 mixed queries in the plain and in the WithLine form (kfdb_scenes.random_scene), each batch one olf_kfdb_detect call"""
    scene = S.random_scene(seed, n_queries=17)
    want, want_state = S.run_reference(scene)
    assert all(len(op) == 17 for op in want) and sum(len(c) for op in want for c in op) > 50
    got, got_state = S.run_library(scene, "detect", context=ctx)
    assert got == want
    assert S.same_state(got_state, want_state)


def test_members_take_one_query_or_a_list(ctx):
    db = KeyFrameDatabase(64, 32, context=ctx)
    a = db.add(S.u(range(10)), S.u(range(4)))
    b = db.add(S.u(range(20, 30)), S.u(range(8, 12)))
    q = lambda i, lo: Query(i, S.u(range(lo, lo + 10)), S.u(range(0, 4)), 10, 10)
    assert db.DetectRelocalizationCandidates(q(1, 0)) == [a]
    assert db.DetectRelocalizationCandidates([q(2, 0), q(3, 20)]) == [[a], [b]]
    assert db.DetectRelocalizationCandidatesWithLine(q(4, 20)) == [a, b]        # a through its lines only
    assert db.DetectLoopCandidates(q(1, 0), 0.5) == [a] and db.DetectLoopCandidatesWithLine([q(2, 0)], [0.5]) == [[a]]
    db.close()


# ---- the pair list ------------------------------------------------------------------------------------------------------------------------------------
def test_score_pairs_equal_restatement(ctx):
    rng = np.random.default_rng(21)
    db, kfs, slots = build(ctx, rng, 40)
    queries = [vector(rng, n) for n in (0, 1, 64, 65, 257, 2000, 300)]
    pairs = np.stack([rng.integers(0, 40, 100), rng.integers(0, 40, 100)], 1).astype(np.int32)
    got = db.score_pairs(pairs)
    want = np.array([R.l1_score(slots[a], slots[b]) for a, b in pairs])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and (want > 0).sum() > 30
    qpairs = np.stack([rng.integers(0, len(queries), 100), rng.integers(0, 40, 100)], 1).astype(np.int32)
    got = db.score_pairs(qpairs, queries=queries)
    want = np.array([R.l1_score(as_list(queries[a]), slots[b]) for a, b in qpairs])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # an index out of range scores NaN and reads nothing
    got = db.score_pairs(np.array([[0, 40], [-1, 0], [3, 4]], np.int32))
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == R.l1_score(slots[3], slots[4])
    db.close()


def test_vocabulary_score(ctx):
    """TemplatedVocabulary::score: the hand-worked pair of test_kfdb_cpu.py (0.25), -0.0 for disjoint vectors, and a 2000-word pair"""
    voc = ORBVocabulary(ctx)
    assert voc.score({1: 0.5, 2: 0.25, 3: 0.25}, {3: 0.5, 7: 0.25, 9: 0.25}) == 0.25
    s = voc.score({1: 1.0}, {})
    assert s == 0.0 and np.signbit(s)
    rng = np.random.default_rng(2)
    a, b = vector(rng, 2000), vector(rng, 2000)
    assert np.float64(voc.score(a, b)).view(np.uint64) == np.float64(R.l1_score(as_list(a), as_list(b))).view(np.uint64)


# ---- refusals: the code comes back and nothing is launched --------------------------------------------------------------------------------------------
def _raw_tables_call(db, n_queries, off, n_slots):
    """olf_kfdb_tables_dev with table buffers of the full size whose heads hold a sentinel: (return code, the sentinel is still there)"""
    import torch
    ids, vals = torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda")
    cells = n_queries * n_slots
    tabs = [torch.empty(cells, dtype=torch.int32, device="cuda"), torch.empty(cells, dtype=torch.int32, device="cuda"), torch.empty(cells, dtype=torch.float64, device="cuda")]
    for t in tabs:
        t[:1024] = 77
    csr, tc = _lib.BowCsrC(off.ctypes.data, ids.data_ptr(), vals.data_ptr()), _lib.KfdbTablesC(*[t.data_ptr() for t in tabs])
    torch.cuda.synchronize()
    rc = lib().olf_kfdb_tables_dev(db._h, n_queries, C.byref(csr), None, C.byref(tc), None, None)
    torch.cuda.synchronize()
    return rc, all(bool((t[:1024] == 77).all()) for t in tabs)


def test_capacity_refusals_launch_nothing(ctx):
    db = KeyFrameDatabase(10000, context=ctx)
    for _ in range(64):
        db.add({1: 1.0})
    rc, untouched = _raw_tables_call(db, 16, np.array([0] * 16 + [_lib.KFDB_MAX_WORDS + 1], np.int32), 64)       # one query of 4097 words
    assert rc == OLF_ERR_CAPACITY and "OLF_KFDB_MAX_WORDS" in last_error() and untouched
    n_queries = _lib.KFDB_MAX_CELLS // 64 + 1                                                                      # Q x slots one row past 2^26
    rc, untouched = _raw_tables_call(db, n_queries, np.zeros(n_queries + 1, np.int32), 64)
    assert rc == OLF_ERR_CAPACITY and "OLF_KFDB_MAX_CELLS" in last_error() and untouched
    with pytest.raises(_lib.OlfError) as e:
        db.detect(S.RELOC, [Query(1, (np.arange(4097), np.full(4097, 1 / 4097)))])
    assert e.value.code == OLF_ERR_CAPACITY and (db.state()["mRelocScore"] == 0).all()
    rc, untouched = _raw_tables_call(db, 16, np.array([0] * 15 + [2, 1], np.int32), 64)                            # offsets that decrease
    assert rc == OLF_ERR_INVALID and untouched
    db.close()


def test_unsupported_scoring_is_refused_with_a_context(ctx):
    h = C.c_void_p()
    for sp, nl, sl in ((1, 0, 0), (0, 10, 2)):
        assert lib().olf_kfdb_create(ctx.handle, 100, nl, sp, sl, C.byref(h)) == OLF_ERR_INVALID and "L1_NORM" in last_error() and not h.value
    voc = ORBVocabulary.from_arrays(2, 1, [0, 0, 0], [0, 1, 1], np.zeros((3, 32), np.uint8), [0, 1, 1], scoring=1, context=ctx)
    with pytest.raises(_lib.OlfError):
        KeyFrameDatabase(voc, context=ctx)
    with pytest.raises(NotImplementedError):
        voc.score({1: 1.0}, {1: 1.0})


# ---- the adaptor ----------------------------------------------------------------------------------------------------------------------------------------
def test_adaptor_kfdb(tmp_path):
    """KeyFrameDatabaseOf<KeyFrame, Frame> over stand-in types gives the candidates worked out in tests/adaptor_kfdb.cpp"""
    exe = str(tmp_path / "adaptor_kfdb")
    libdir = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "adaptor_kfdb.cpp"), "-L" + libdir, "-lorbline_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert out.returncode == 0 and b"ADAPTOR_KFDB_OK" in out.stdout, out.stdout
