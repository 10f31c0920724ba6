"""olf_search_by_bow_pairs_dev without a device: the argument checks come before anything touches one, and every scenario of bow_pairs_scenes.py
proves from the oracle (or a numpy count) that its case occurs."""
import ctypes as C
import pytest
import bow_pairs_scenes as S
from orb_line_slam_amd import _lib
from orb_line_slam_amd._lib import OLF_ERR_INVALID, last_error, lib


def test_null_context_is_refused():
    assert lib().olf_search_by_bow_pairs_dev(None, None, None, 2, 1, None, None, 0, 0.7, 1, 4, None, None, None) == OLF_ERR_INVALID
    assert "olf_search_by_bow_pairs_dev" in last_error()


def test_bad_arguments_are_refused_before_the_context_is_looked_at():
    """the context and the vocabulary handed over here are not ones: a call that got past its argument checks would read them"""
    buf = (C.c_uint8 * 64)()
    a = C.cast(buf, C.c_void_p)

    def call(form=0, n_frames=2, n_pairs=1, levelsup=4, pairs=a, m=a, n=a, **edit):
        tb = _lib.TrackBatchC()
        tb.kps, tb.desc, tb.counts, tb.img_stride = a, a, a, 1
        for k, v in edit.items():
            setattr(tb, k, v)
        return lib().olf_search_by_bow_pairs_dev(a, a, C.byref(tb), n_frames, n_pairs, pairs, None, form, 0.7, 1, levelsup, m, n, None)

    for form in (-1, 2):
        assert call(form=form) == OLF_ERR_INVALID                      # an unknown form
    assert call(n_frames=-1) == OLF_ERR_INVALID and call(n_pairs=-1) == OLF_ERR_INVALID and call(levelsup=-1) == OLF_ERR_INVALID
    assert call(pairs=None) == OLF_ERR_INVALID and call(m=None) == OLF_ERR_INVALID and call(n=None) == OLF_ERR_INVALID
    for k in ("kps", "desc", "counts"):
        assert call(**{k: None}) == OLF_ERR_INVALID, k
    assert call(img_stride=0) == OLF_ERR_INVALID
    assert "olf_search_by_bow_pairs_dev" in last_error()


@pytest.mark.parametrize("fn,args", S.ALL_SCENARIOS, ids=lambda v: getattr(v, "__name__", "-".join(str(int(x)) for x in v) if isinstance(v, tuple) else None))
def test_scenario_occurs(fn, args):
    fn(*args)
