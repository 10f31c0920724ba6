"""olf_search_by_sim3_pairs_dev without a device: the argument checks come before anything touches one."""
import ctypes as C
import pytest
from orb_line_slam_amd import _lib
from orb_line_slam_amd._lib import OLF_ERR_INVALID, last_error, lib

WHO = "olf_search_by_sim3_pairs_dev"
TB_REQUIRED = ("kps", "desc", "counts", "cell_offsets", "cell_index", "Tcw", "mp_world")
ARG_REQUIRED = ("maxd", "mind", "pairs", "s12", "R12", "t12", "matches12", "nfound")


def _args():
    """a complete argument block: every pointer names one readable buffer (none is read before the checks are through), valid bounds"""
    buf = (C.c_uint8 * 256)()
    a = C.cast(buf, C.c_void_p)
    tb = _lib.TrackBatchC()
    for k in TB_REQUIRED:
        setattr(tb, k, a)
    tb.img_stride, tb.minX, tb.maxX, tb.minY, tb.maxY = 1, 0.0, 320.0, 0.0, 240.0
    return buf, tb, {k: a for k in ARG_REQUIRED}


def _call(ctx, tb, p, n_frames=2, n_pairs=1):
    g = lambda k: p.get(k)
    return lib().olf_search_by_sim3_pairs_dev(ctx, tb, n_frames, None, g("maxd"), g("mind"), n_pairs, g("pairs"), g("s12"), g("R12"), g("t12"), 7.5,
                                              g("matches12"), None, None, g("nfound"), None)


def test_null_context_is_refused():
    buf, tb, p = _args()
    assert _call(None, C.byref(tb), p) == OLF_ERR_INVALID
    assert WHO in last_error()
    assert _call(None, None, {}) == OLF_ERR_INVALID and WHO in last_error()


def test_null_batch_is_refused():
    buf, tb, p = _args()
    assert _call(C.cast(buf, C.c_void_p), None, p) == OLF_ERR_INVALID and WHO in last_error()


@pytest.mark.parametrize("name", ARG_REQUIRED)
def test_null_required_argument_is_refused_before_the_context_is_looked_at(name):
    """the context handed over here is not one: a call that got past its argument checks would read it"""
    buf, tb, p = _args()
    p[name] = None
    assert _call(C.cast(buf, C.c_void_p), C.byref(tb), p) == OLF_ERR_INVALID
    assert WHO in last_error()


@pytest.mark.parametrize("name", TB_REQUIRED)
def test_null_required_batch_pointer_is_refused(name):
    buf, tb, p = _args()
    setattr(tb, name, None)
    assert _call(C.cast(buf, C.c_void_p), C.byref(tb), p) == OLF_ERR_INVALID
    assert WHO in last_error()


def test_negative_counts_and_a_zero_stride_are_refused():
    buf, tb, p = _args()
    fake = C.cast(buf, C.c_void_p)
    assert _call(fake, C.byref(tb), p, n_frames=-1) == OLF_ERR_INVALID and WHO in last_error()
    assert _call(fake, C.byref(tb), p, n_pairs=-1) == OLF_ERR_INVALID and WHO in last_error()
    tb.img_stride = 0
    assert _call(fake, C.byref(tb), p) == OLF_ERR_INVALID and WHO in last_error()


@pytest.mark.parametrize("bounds", [(0.0, 0.0, 0.0, 240.0), (320.0, 0.0, 0.0, 240.0), (0.0, 320.0, 240.0, 240.0), (0.0, 320.0, 240.0, 0.0)])
def test_inverted_bounds_are_refused(bounds):
    buf, tb, p = _args()
    tb.minX, tb.maxX, tb.minY, tb.maxY = bounds
    assert _call(C.cast(buf, C.c_void_p), C.byref(tb), p) == OLF_ERR_INVALID
    assert WHO in last_error()


def test_the_gpu_scenarios_hold(oracle):
    """A check of the fixtures, not of the entry (it needs only the oracle): tests/sim3_pairs_scenes.py on the CPU -- the seed and the hand-built cases
    give what tests/test_sim3_pairs_gpu.py relies on (each scenario asserts it)"""
    import sim3_pairs_scenes as S
    cap = 1432
    s = S.scenario_batch(cap)
    assert len(s.pairs) >= 12 and set(s.exp) == {7.5, 10.0}
    assert len(S.scenario_gates(cap)) >= 9
    assert S.scenario_counts(cap).exp[3][1] >= 20
