"""olf_fuse_search_batch_dev without a device: the argument checks come before anything touches one."""
import ctypes as C
from orb_line_slam_amd import _lib
from orb_line_slam_amd._lib import OLF_ERR_INVALID, last_error, lib


def _call(ctx, tb, lm, n_frames=2, bi=1, bd=1):
    out = (C.c_int32 * 8)()
    p = C.cast(out, C.c_void_p)
    return lib().olf_fuse_search_batch_dev(ctx, tb, n_frames, lm, None, None, None, 3.0, p if bi else None, p if bd else None, None, None)


def _args():
    """a complete argument block: every pointer names one readable buffer (none is read before the checks are through), valid bounds, no entries"""
    buf = (C.c_uint8 * 64)()
    a = C.cast(buf, C.c_void_p)
    tb, lm = _lib.TrackBatchC(), _lib.LocalMapC()
    for k in ("kps", "desc", "counts", "uright", "cell_offsets", "cell_index", "Tcw"):
        setattr(tb, k, a)
    tb.img_stride, tb.minX, tb.maxX, tb.minY, tb.maxY = 1, 0.0, 320.0, 0.0, 240.0
    for k in ("world", "normal", "maxd", "mind", "desc", "bad"):
        setattr(lm, k, a)
    lm.n_mp = 4
    return buf, tb, lm


def test_null_context_is_refused():
    buf, tb, lm = _args()
    assert _call(None, C.byref(tb), C.byref(lm)) == OLF_ERR_INVALID
    assert "olf_fuse_search_batch_dev" in last_error()
    assert lib().olf_fuse_search_batch_dev(None, None, 2, None, None, None, None, 3.0, None, None, None, None) == OLF_ERR_INVALID


def test_null_required_pointers_are_refused_before_the_context_is_looked_at():
    """the context handed over here is not one: a call that got past its argument checks would read it"""
    buf, tb, lm = _args()
    fake = C.cast(buf, C.c_void_p)
    assert _call(fake, None, C.byref(lm)) == OLF_ERR_INVALID and _call(fake, C.byref(tb), None) == OLF_ERR_INVALID
    assert _call(fake, C.byref(tb), C.byref(lm), bi=0) == OLF_ERR_INVALID and _call(fake, C.byref(tb), C.byref(lm), bd=0) == OLF_ERR_INVALID
    assert _call(fake, C.byref(tb), C.byref(lm), n_frames=-1) == OLF_ERR_INVALID
    for k in ("kps", "desc", "counts", "uright", "cell_offsets", "cell_index", "Tcw"):
        _, t2, _ = _args()
        setattr(t2, k, None)
        assert _call(fake, C.byref(t2), C.byref(lm)) == OLF_ERR_INVALID, k
    for k in ("world", "normal", "maxd", "mind", "desc", "bad"):
        _, _, l2 = _args()
        setattr(l2, k, None)
        assert _call(fake, C.byref(tb), C.byref(l2)) == OLF_ERR_INVALID, k
    _, t2, _ = _args()
    t2.maxX = 0.0
    assert _call(fake, C.byref(t2), C.byref(lm)) == OLF_ERR_INVALID
    _, _, l2 = _args()
    l2.n_mp = -1
    assert _call(fake, C.byref(tb), C.byref(l2)) == OLF_ERR_INVALID
