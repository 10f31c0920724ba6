"""The key-frame database without a device: known answers worked out by hand, olf_kfdb_select against the restatement (kfdb_reference.py) over the scenes of
kfdb_scenes.py, the argument checks of every new entry, the selection code as a stand-alone program under AddressSanitizer / UBSan, and the adaptor."""
import ctypes as C
import os
import struct
import subprocess
import numpy as np
import pytest
import kfdb_reference as R
import kfdb_scenes as S
from orb_line_slam_amd import _lib
from orb_line_slam_amd._lib import OLF_ERR_CAPACITY, OLF_ERR_INVALID, OLF_OK, last_error, lib
from orb_line_slam_amd.database import KeyFrameDatabase, Query

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# ---- (a) known answers ------------------------------------------------------------------------------------------------------------------------------
def test_score_of_one_common_word():
    """v1 = {1: .5, 2: .25, 3: .25}, v2 = {3: .5, 7: .25, 9: .25}: the one common word is 3 with vi = .25, wi = .5, so the sum is
    |.25 - .5| - |.25| - |.5| = -.5 and the score -(-.5) / 2 = .25 = 0x3FD0000000000000, every step exact in binary"""
    v1, v2 = [(1, 0.5), (2, 0.25), (3, 0.25)], [(3, 0.5), (7, 0.25), (9, 0.25)]
    assert bits(R.l1_score(v1, v2)) == 0x3FD0000000000000 and bits(R.l1_score(v2, v1)) == 0x3FD0000000000000
    t = R.tables([v1], [v2])
    assert t["common"][0, 0] == 1 and t["first"][0, 0] == 3 and bits(float(t["score"][0, 0])) == 0x3FD0000000000000


def test_score_of_disjoint_vectors_is_minus_zero():
    """no common word: score stays +0.0 and -score / 2.0 is -0.0 = 0x8000000000000000 (ScoringObject.cpp:65)"""
    s = R.l1_score([(1, 0.5), (2, 0.5)], [(3, 0.5), (4, 0.5)])
    assert s == 0.0 and bits(s) == 0x8000000000000000
    assert bits(R.l1_score([], [(3, 1.0)])) == 0x8000000000000000 and bits(R.l1_score([], [])) == 0x8000000000000000
    assert bits(float(R.tables([[(1, 1.0)]], [[]])["score"][0, 0])) == 0x8000000000000000


def _select_counts(counts):
    """a relocalisation query against len(counts) key frames with these common-word counts (every score 0.5): which slots were scored (their mRelocScore
    is written), from olf_kfdb_select and from the arithmetic of :438 alone"""
    n = len(counts)
    db = KeyFrameDatabase(1000)
    for k in range(n):
        db.add({k: 1.0})
    t = {"common": np.array([counts], np.int32), "first": np.zeros((1, n), np.int32), "score": np.full((1, n), 0.5)}
    db.select(S.RELOC, [Query(1, {})], t)
    scored = (db.state()["mRelocScore"] == np.float32(0.5)).tolist()
    db.close()
    return scored


@pytest.mark.parametrize("max_common,min_common", [(5, 4), (6, 4), (10, 8)])
def test_min_common_words(max_common, min_common):
    """minCommonWords = maxCommonWords * 0.8f truncated: 5 * 0.8f = 4.0000000596 rounds to the float 4.0 -> 4; 6 * 0.8f = 4.8000002 -> 4;
    10 * 0.8f = 8.0000001192 rounds to 8.0 -> 8.  A key frame is scored when its count is strictly greater: the one with exactly minCommonWords is not."""
    assert int(np.float32(max_common) * np.float32(0.8)) == min_common
    counts = [max_common, min_common, min_common + 1]
    assert _select_counts(counts) == [True, False, True]
    # and the restatement agrees: three key frames sharing max_common, min_common and min_common + 1 of the query's words
    s = S.Scene(1000, 0)
    q = {w: 0.01 for w in range(max_common)}
    for i, c in enumerate(counts):
        s.add(f"k{i}", {**{w: 0.01 for w in range(c)}, **{500 + 20 * i + w: 0.01 for w in range(3)}})
    s.query(S.RELOC, [dict(mnId=1, bow=q)])
    _, state = S.run_reference(s)
    assert (state["mRelocScore"] != 0).tolist() == [True, False, True]


# ---- (b) olf_kfdb_select against the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scenario", S.ALL_SCENARIOS, ids=lambda f: f.__name__)
def test_select_equals_restatement(scenario):
    scene = scenario()                                   # (asserts that its case occurs)
    want, want_state, tables = S.run_reference(scene, want_tables=True)
    got, got_state = S.run_library(scene, "select", tables=tables)
    assert got == want
    assert S.same_state(got_state, want_state)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_select_equals_restatement_on_random_batches(seed):
    scene = S.random_scene(seed)
    want, want_state, tables = S.run_reference(scene, want_tables=True)
    assert sum(len(c) for op in want for c in op) > 50 and any(len(c) > 1 for op in want for c in op)
    got, got_state = S.run_library(scene, "select", tables=tables)
    assert got == want
    assert S.same_state(got_state, want_state)


def test_without_line_vocabulary_the_withline_forms_return_nothing():
    """:232-235, :516-519"""
    s = S.Scene(64, 0).add("A", S.u(range(10)), S.u(range(4)))
    s.query(S.RELOC_LINE, [dict(mnId=1, bow=S.u(range(10)), bow_l=S.u(range(4)), N=1, N_l=1)]).query(S.LOOP_LINE, [dict(mnId=1, bow=S.u(range(10)), N=1, N_l=1)], 0.0)
    s.query(S.RELOC, [dict(mnId=2, bow=S.u(range(10)))])
    want, want_state, tables = S.run_reference(s, want_tables=True)
    assert want == [[[]], [[]], [[0]]]
    got, got_state = S.run_library(s, "select", tables=tables)
    assert got == want and S.same_state(got_state, want_state)


def test_add_erase_clear_and_size():
    db = KeyFrameDatabase(100, 50)
    assert db.size() == (0, 0)
    assert [db.add({1: 0.5, 5: 0.5}, {2: 1.0}), db.add({}), db.add({7: 1.0})] == [0, 1, 2]
    db.erase(1); db.erase(1)
    assert db.size() == (3, 2)
    assert db.add({3: 1.0}) == 3                        # a slot is not reused
    db.clear()
    assert db.size() == (0, 0) and db.add({3: 1.0}) == 0
    for bad in ({5: 0.5, 100: 0.5}, ([3, 3], [0.5, 0.5]), ([4, 3], [0.5, 0.5]), ([-1], [1.0])):
        with pytest.raises(_lib.OlfError) as e:
            db.add(bad)
        assert e.value.code == OLF_ERR_INVALID
    big = KeyFrameDatabase(10000)
    with pytest.raises(_lib.OlfError) as e:
        big.add((np.arange(_lib.KFDB_MAX_WORDS + 1), np.ones(_lib.KFDB_MAX_WORDS + 1)))
    assert e.value.code == OLF_ERR_CAPACITY and "OLF_KFDB_MAX_WORDS" in last_error()
    with pytest.raises(_lib.OlfError):
        db.erase(7)


def test_slot_limit_is_refused():
    """slots are not reused, so a database holds OLF_KFDB_MAX_SLOTS key frames between two clears: the next add returns OLF_ERR_CAPACITY and names the limit"""
    h, slot = C.c_void_p(), C.c_int32()
    assert lib().olf_kfdb_create(None, 10, 0, 0, 0, C.byref(h)) == OLF_OK
    add, ref = lib().olf_kfdb_add, C.byref(slot)
    for _ in range(_lib.KFDB_MAX_SLOTS):
        add(h, None, None, 0, None, None, 0, ref)
    assert slot.value == _lib.KFDB_MAX_SLOTS - 1
    assert add(h, None, None, 0, None, None, 0, ref) == OLF_ERR_CAPACITY and "OLF_KFDB_MAX_SLOTS" in last_error()
    assert lib().olf_kfdb_clear(h) == OLF_OK and add(h, None, None, 0, None, None, 0, ref) == OLF_OK and slot.value == 0
    lib().olf_kfdb_destroy(h)


def test_unsupported_scoring_is_refused():
    h = C.c_void_p()
    for sp, nl, sl in ((1, 0, 0), (0, 10, 3), (5, 10, 0)):
        assert lib().olf_kfdb_create(None, 100, nl, sp, sl, C.byref(h)) == OLF_ERR_INVALID
        assert "L1_NORM" in last_error() and not h.value
    assert lib().olf_kfdb_create(None, 100, 0, 0, 4, C.byref(h)) == OLF_OK            # no line vocabulary: its scoring is not looked at
    lib().olf_kfdb_destroy(h)


def test_select_refuses_more_candidates_than_capacity_and_changes_nothing():
    db = KeyFrameDatabase(100)
    db.add({1: 1.0}); db.add({1: 1.0})
    n, ids = 2, np.array([1], np.int64)
    t = [np.array([[1, 1]], np.int32), np.array([[1, 1]], np.int32), np.array([[1.0, 1.0]])]
    tc = _lib.KfdbTablesC(*[a.ctypes.data for a in t])
    nb_off, off, cand = np.zeros(n + 1, np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)
    args = lambda cap: (db._h, S.RELOC, 1, _lib.ptr(ids), None, None, None, None, None, _lib.ptr(nb_off), None, n, C.byref(tc), None, _lib.ptr(off), _lib.ptr(cand), cap)
    assert lib().olf_kfdb_select(*args(1)) == OLF_ERR_CAPACITY
    assert (db.state()["mRelocScore"] == 0).all()
    assert lib().olf_kfdb_select(*args(2)) == OLF_OK and off.tolist() == [0, 2] and cand.tolist() == [0, 1]      # the id was not used up by the refusal
    assert (db.state()["mRelocScore"] == 1).all()
    bad_nb = np.array([0, 1, 1], np.int32)
    ids[0] = 2
    a = list(args(2)); a[9] = _lib.ptr(bad_nb); a[10] = _lib.ptr(np.array([2], np.int32))
    assert lib().olf_kfdb_select(*a) == OLF_ERR_INVALID and "neighbour" in last_error()


# ---- (c) argument checks: handles that are not handles -----------------------------------------------------------------------------------------------
def test_null_handles_are_refused():
    L = lib()
    assert L.olf_kfdb_create(None, 100, 0, 0, 0, None) == OLF_ERR_INVALID and "olf_kfdb_create" in last_error()
    assert L.olf_kfdb_add(None, None, None, 0, None, None, 0, None) == OLF_ERR_INVALID and "olf_kfdb_add" in last_error()
    assert L.olf_kfdb_erase(None, 0) == OLF_ERR_INVALID and "olf_kfdb_erase" in last_error()
    assert L.olf_kfdb_clear(None) == OLF_ERR_INVALID and "olf_kfdb_clear" in last_error()
    assert L.olf_kfdb_size(None, None, None) == OLF_ERR_INVALID and "olf_kfdb_size" in last_error()
    assert L.olf_kfdb_state(None, None, None, None) == OLF_ERR_INVALID and "olf_kfdb_state" in last_error()
    assert L.olf_kfdb_tables_dev(None, 1, None, None, None, None, None) == OLF_ERR_INVALID and "olf_kfdb_tables_dev" in last_error()
    assert L.olf_kfdb_select(None, 0, 0, *([None] * 8), 0, None, None, None, None, 0) == OLF_ERR_INVALID and "olf_kfdb_select" in last_error()
    assert L.olf_kfdb_detect(None, 0, 0, None, None, None, *([None] * 9), 0) == OLF_ERR_INVALID and "olf_kfdb_detect" in last_error()
    assert L.olf_bow_score_pairs_dev(None, 0, 0, None, None, 0, None, None) == OLF_ERR_INVALID and "olf_bow_score_pairs_dev" in last_error()
    assert L.olf_bow_score(None, None, None, 0, None, None, 0, None) == OLF_ERR_INVALID and "olf_bow_score" in last_error()
    L.olf_kfdb_destroy(None)


def test_bad_arguments_are_refused_before_the_handles_are_looked_at():
    """the context and the database handed over here are not ones: a call that got past its argument checks would read them"""
    L = lib()
    buf = (C.c_uint8 * 256)()
    a = C.cast(buf, C.c_void_p)
    h = C.c_void_p()
    for args in ((0, 0, 0, 0), (100, -1, 0, 0), (100, 0, 1, 0), (100, 10, 0, 2)):
        assert L.olf_kfdb_create(a, *args, C.byref(h)) == OLF_ERR_INVALID
    assert L.olf_kfdb_create(a, 100, 0, 0, 0, None) == OLF_ERR_INVALID
    slot = C.c_int32()
    assert L.olf_kfdb_add(a, a, a, -1, a, a, 0, C.byref(slot)) == OLF_ERR_INVALID and L.olf_kfdb_add(a, a, a, 1, a, a, 0, None) == OLF_ERR_INVALID
    assert L.olf_kfdb_add(a, None, a, 1, a, a, 0, C.byref(slot)) == OLF_ERR_INVALID and L.olf_kfdb_add(a, a, a, 1, a, None, 1, C.byref(slot)) == OLF_ERR_INVALID
    csr, bad_csr = _lib.BowCsrC(a, a, a), _lib.BowCsrC(a, None, a)
    tab, bad_tab = _lib.KfdbTablesC(a, a, a), _lib.KfdbTablesC(a, a, None)
    T = L.olf_kfdb_tables_dev
    assert T(a, -1, C.byref(csr), None, C.byref(tab), None, None) == OLF_ERR_INVALID
    assert T(a, 1, None, None, C.byref(tab), None, None) == OLF_ERR_INVALID and T(a, 1, C.byref(bad_csr), None, C.byref(tab), None, None) == OLF_ERR_INVALID
    assert T(a, 1, C.byref(csr), None, C.byref(bad_tab), None, None) == OLF_ERR_INVALID and T(a, 1, C.byref(csr), C.byref(csr), C.byref(tab), None, None) == OLF_ERR_INVALID
    assert T(a, 1, C.byref(csr), None, C.byref(tab), C.byref(tab), None) == OLF_ERR_INVALID and "olf_kfdb_tables_dev" in last_error()

    def select(form=0, nq=1, ids=a, np_=a, nl=a, ms=a, conn_off=None, conn=None, nb_off=a, n_slots=1, tp=tab, tl=tab, off=a, cand=a, cap=1):
        return L.olf_kfdb_select(a, form, nq, ids, np_, nl, ms, conn_off, conn, nb_off, a, n_slots, C.byref(tp) if tp else None, C.byref(tl) if tl else None, off, cand, cap)

    for form in (-1, 4):
        assert select(form=form) == OLF_ERR_INVALID
    assert select(nq=-1) == OLF_ERR_INVALID and select(n_slots=-1) == OLF_ERR_INVALID and select(cap=-1) == OLF_ERR_INVALID
    assert select(ids=None) == OLF_ERR_INVALID and select(nb_off=None) == OLF_ERR_INVALID and select(off=None) == OLF_ERR_INVALID and select(cand=None) == OLF_ERR_INVALID
    assert select(form=0, ms=None) == OLF_ERR_INVALID and select(form=1, np_=None) == OLF_ERR_INVALID and select(form=3, nl=None) == OLF_ERR_INVALID
    assert select(tp=None) == OLF_ERR_INVALID and select(tp=bad_tab) == OLF_ERR_INVALID and select(form=1, tl=None) == OLF_ERR_INVALID
    assert select(conn_off=a, conn=None) == OLF_ERR_INVALID and "olf_kfdb_select" in last_error()

    def detect(form=0, nq=1, ids=a, qp=csr, ql=csr, np_=a, nl=a, ms=a, conn_off=None, conn=None, nb_off=a, off=a, cand=a, cap=1):
        return L.olf_kfdb_detect(a, form, nq, ids, C.byref(qp) if qp else None, C.byref(ql) if ql else None, np_, nl, ms, conn_off, conn, nb_off, a, off, cand, cap)

    for form in (-1, 4):
        assert detect(form=form) == OLF_ERR_INVALID
    assert detect(nq=-1) == OLF_ERR_INVALID and detect(cap=-1) == OLF_ERR_INVALID and detect(ids=None) == OLF_ERR_INVALID and detect(qp=None) == OLF_ERR_INVALID
    assert detect(form=1, ql=None) == OLF_ERR_INVALID and detect(form=1, ms=None) == OLF_ERR_INVALID and detect(form=3, np_=None) == OLF_ERR_INVALID
    assert detect(nb_off=None) == OLF_ERR_INVALID and detect(off=None) == OLF_ERR_INVALID and detect(cand=None) == OLF_ERR_INVALID
    assert detect(conn_off=a, conn=None) == OLF_ERR_INVALID and "olf_kfdb_detect" in last_error()
    P = L.olf_bow_score_pairs_dev
    assert P(a, 2, 1, a, None, 0, a, None) == OLF_ERR_INVALID and P(a, 0, -1, a, None, 0, a, None) == OLF_ERR_INVALID and P(a, 0, 1, None, None, 0, a, None) == OLF_ERR_INVALID
    assert P(a, 0, 1, a, None, 0, None, None) == OLF_ERR_INVALID and P(a, 0, 1, a, C.byref(bad_csr), 1, a, None) == OLF_ERR_INVALID and P(a, 0, 1, a, None, -1, a, None) == OLF_ERR_INVALID
    assert "olf_bow_score_pairs_dev" in last_error()
    out = C.c_double()
    ids, vals = np.array([3, 2], np.int32), np.ones(2)
    assert L.olf_bow_score(a, _lib.ptr(ids), _lib.ptr(vals), 2, None, None, 0, C.byref(out)) == OLF_ERR_INVALID          # ids not ascending
    assert L.olf_bow_score(a, None, None, 1, None, None, 0, C.byref(out)) == OLF_ERR_INVALID and L.olf_bow_score(a, None, None, 0, None, None, -1, C.byref(out)) == OLF_ERR_INVALID
    assert L.olf_bow_score(a, None, None, 0, None, None, 0, None) == OLF_ERR_INVALID and "olf_bow_score" in last_error()


def test_a_database_without_a_context_refuses_the_device_entries():
    db = KeyFrameDatabase(100)
    db.add({1: 1.0})
    off, one = np.zeros(2, np.int32), np.zeros(1, np.int64)
    csr, tab = _lib.BowCsrC(off.ctypes.data, one.ctypes.data, one.ctypes.data), _lib.KfdbTablesC(*[one.ctypes.data] * 3)
    assert lib().olf_kfdb_tables_dev(db._h, 1, C.byref(csr), None, C.byref(tab), None, None) == OLF_ERR_INVALID and "without a context" in last_error()
    assert lib().olf_bow_score_pairs_dev(db._h, 0, 1, one.ctypes.data, None, 0, one.ctypes.data, None) == OLF_ERR_INVALID and "without a context" in last_error()
    with pytest.raises(_lib.OlfError) as e:
        db.detect(S.RELOC, [Query(1, {1: 1.0})])
    assert e.value.code == OLF_ERR_INVALID and "without a context" in str(e.value)


# ---- (d) the selection code under sanitizers, in its own process --------------------------------------------------------------------------------------
def test_select_stand_alone_under_sanitizers(tmp_path):
    exe = str(tmp_path / "kfdb_select_main")
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-o", str(tmp_path / "probe"), "-"], input=b"int main() { return 0; }\n",
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if probe.returncode != 0:
        pytest.skip("this g++ has no AddressSanitizer / UBSan runtime: " + probe.stdout.decode()[-300:])
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "kfdb_select_main.cpp"), os.path.join(ROOT, "orb_line_slam_amd", "csrc", "kfdb_host.cpp")], check=True)
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert out.returncode == 0 and b"KFDB_SELECT_OK" in out.stdout, out.stdout.decode()[-3000:]


# ---- (e) the adaptor ------------------------------------------------------------------------------------------------------------------------------------
def test_adaptor_compiles_and_instantiates(tmp_path):
    """KeyFrameDatabaseOf<KeyFrame, Frame> and ORBVocabulary::score against stand-in types: every member is instantiated.  The program needs a device to
    do more than that; tests/test_kfdb_gpu.py runs it where there is one."""
    exe = str(tmp_path / "adaptor_kfdb")
    libdir = os.path.join(ROOT, "orb_line_slam_amd", "csrc")
    subprocess.run(["g++", "-std=c++11", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "adaptor_kfdb.cpp"), "-L" + libdir, "-lorbline_hip",
                    "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert os.path.exists(exe)
