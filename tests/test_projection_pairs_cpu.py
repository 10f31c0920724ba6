"""olf_search_by_projection_kf_pairs_dev and olf_search_by_projection_sim3_batch_dev without a device: the argument checks come before anything touches
one; and the fixtures of tests/test_projection_pairs_gpu.py hold on the CPU oracle."""
import ctypes as C
import pytest
from orb_line_slam_amd import _lib
from orb_line_slam_amd._lib import OLF_ERR_INVALID, last_error, lib

RELOC, LOOP = "olf_search_by_projection_kf_pairs_dev", "olf_search_by_projection_sim3_batch_dev"
TB_REQUIRED = {RELOC: ("kps", "desc", "counts", "cell_offsets", "cell_index", "Tcw", "mp_world"), LOOP: ("kps", "desc", "counts", "cell_offsets", "cell_index")}
ARG_REQUIRED = {RELOC: ("maxd", "mind", "pairs", "matches", "nmatches"), LOOP: ("Scw", "frame_matched", "nmatches")}
MAP_REQUIRED = ("world", "normal", "maxd", "mind", "desc", "bad")
CASES = [(w, k) for w in (RELOC, LOOP) for k in ARG_REQUIRED[w]]
TB_CASES = [(w, k) for w in (RELOC, LOOP) for k in TB_REQUIRED[w]]


def _args(who):
    """a complete argument block: every pointer names one readable buffer (none is read before the checks are through), valid bounds"""
    buf = (C.c_uint8 * 256)()
    a = C.cast(buf, C.c_void_p)
    tb = _lib.TrackBatchC()
    for k in TB_REQUIRED[who]:
        setattr(tb, k, a)
    tb.img_stride, tb.minX, tb.maxX, tb.minY, tb.maxY = 1, 0.0, 320.0, 0.0, 240.0
    lm = _lib.LocalMapC()
    for k in MAP_REQUIRED:
        setattr(lm, k, a)
    lm.n_mp = 4
    return buf, tb, lm, {k: a for k in ARG_REQUIRED[who]}


def _call(who, ctx, tb, lm, p, n_frames=2, n_pairs=1):
    g = lambda k: p.get(k)
    if who == RELOC:
        return lib().olf_search_by_projection_kf_pairs_dev(ctx, tb, n_frames, None, g("maxd"), g("mind"), n_pairs, g("pairs"), None, None, None, 10.0, None, 100,
                                                           None, 1, g("matches"), g("nmatches"), None)
    return lib().olf_search_by_projection_sim3_batch_dev(ctx, tb, n_frames, lm, g("Scw"), g("frame_matched"), 10.0, None, g("nmatches"), None)


@pytest.mark.parametrize("who", [RELOC, LOOP])
def test_null_context_and_null_batch_are_refused(who):
    buf, tb, lm, p = _args(who)
    fake = C.cast(buf, C.c_void_p)
    assert _call(who, None, C.byref(tb), C.byref(lm), p) == OLF_ERR_INVALID and who in last_error()
    assert _call(who, None, None, None, {}) == OLF_ERR_INVALID and who in last_error()
    assert _call(who, fake, None, C.byref(lm), p) == OLF_ERR_INVALID and who in last_error()
    if who == LOOP:
        assert _call(who, fake, C.byref(tb), None, p) == OLF_ERR_INVALID and who in last_error()


@pytest.mark.parametrize("who,name", CASES)
def test_null_required_argument_is_refused_before_the_context_is_looked_at(who, name):
    """the context handed over here is not one: a call that got past its argument checks would read it"""
    buf, tb, lm, p = _args(who)
    p[name] = None
    assert _call(who, C.cast(buf, C.c_void_p), C.byref(tb), C.byref(lm), p) == OLF_ERR_INVALID
    assert who in last_error()


@pytest.mark.parametrize("who,name", TB_CASES)
def test_null_required_batch_pointer_is_refused(who, name):
    buf, tb, lm, p = _args(who)
    setattr(tb, name, None)
    assert _call(who, C.cast(buf, C.c_void_p), C.byref(tb), C.byref(lm), p) == OLF_ERR_INVALID
    assert who in last_error()


@pytest.mark.parametrize("name", MAP_REQUIRED)
def test_null_map_array_is_refused(name):
    buf, tb, lm, p = _args(LOOP)
    setattr(lm, name, None)
    assert _call(LOOP, C.cast(buf, C.c_void_p), C.byref(tb), C.byref(lm), p) == OLF_ERR_INVALID
    assert LOOP in last_error()


@pytest.mark.parametrize("who", [RELOC, LOOP])
def test_negative_counts_and_a_zero_stride_are_refused(who):
    buf, tb, lm, p = _args(who)
    fake = C.cast(buf, C.c_void_p)
    assert _call(who, fake, C.byref(tb), C.byref(lm), p, n_frames=-1) == OLF_ERR_INVALID and who in last_error()
    if who == RELOC:
        assert _call(who, fake, C.byref(tb), C.byref(lm), p, n_pairs=-1) == OLF_ERR_INVALID and who in last_error()
    else:
        lm.n_mp = -1
        assert _call(who, fake, C.byref(tb), C.byref(lm), p) == OLF_ERR_INVALID and who in last_error()
        lm.n_mp = 4
        lm.list_offsets, lm.n_entries = fake, -1
        assert _call(who, fake, C.byref(tb), C.byref(lm), p) == OLF_ERR_INVALID and who in last_error()
        lm.n_entries = 3                                     # (entries without a list_index)
        assert _call(who, fake, C.byref(tb), C.byref(lm), p) == OLF_ERR_INVALID and who in last_error()
        lm.list_offsets, lm.n_entries = None, 0
    tb.img_stride = 0
    assert _call(who, fake, C.byref(tb), C.byref(lm), p) == OLF_ERR_INVALID and who in last_error()


@pytest.mark.parametrize("who", [RELOC, LOOP])
@pytest.mark.parametrize("bounds", [(0.0, 0.0, 0.0, 240.0), (320.0, 0.0, 0.0, 240.0), (0.0, 320.0, 240.0, 240.0), (0.0, 320.0, 240.0, 0.0)])
def test_inverted_bounds_are_refused(who, bounds):
    buf, tb, lm, p = _args(who)
    tb.minX, tb.maxX, tb.minY, tb.maxY = bounds
    assert _call(who, C.cast(buf, C.c_void_p), C.byref(tb), C.byref(lm), p) == OLF_ERR_INVALID
    assert who in last_error()


def test_the_gpu_scenarios_hold(oracle):
    """A check of the fixtures, not of the entries (it needs only the oracle): tests/projection_pairs_scenes.py on the CPU -- the seed and the hand-built
    cases give what tests/test_projection_pairs_gpu.py relies on (each scenario asserts it)"""
    import projection_pairs_scenes as S
    cap = 1432
    s = S.scenario_reloc_batch(cap)
    n10 = s.exp[(10.0, 1)][1]
    assert len(s.pairs) >= 12 and 2 * int((n10 >= 20).sum()) >= len(s.pairs)                                      # half of the pairs end with >= 20 matches
    assert any((s.exp[(th, 0)][1] > s.exp[(th, 1)][1]).any() for th in S.RELOC_THS)                                # a pair loses matches to the rotation check
    i, first, earlier, got = s.displaced                                                                         # a later point on its second choice
    assert earlier < i and first != got
    gates = {c.name: c for c in S.scenario_reloc_gates(cap)}
    assert list(gates["recompute"].exp[0][0][:5]) == [0, 1, 2, 3, 4]                                             # Q (feature 4) ends on key point 4
    assert gates["negative_depth"].exp[0][1] == 1 and gates["negative_depth"].exp[0][0][0] == 0                  # searched, and matched
    assert gates["rotation_rejected"].exp[1][1] < gates["rotation_rejected"].exp[0][1]
    assert S.scenario_reloc_counts(cap).exp[1][0] >= 20
    t = S.scenario_loop_batch(cap)
    assert set(t.exp) == set(S.LOOP_THS) and 2 * int((t.exp[10][1] >= 20).sum()) >= len(t.kfs)
    assert S.scenario_loop_counts(cap).exp[1][6] >= 20
    lg = {c.name: c for c in S.scenario_loop_gates(cap)}
    assert list(lg["recompute"].exp[0][:5]) == [0, 1, 2, 3, 4] and lg["order_first"].exp[1] == 2 and lg["order_second"].exp[1] == 1
